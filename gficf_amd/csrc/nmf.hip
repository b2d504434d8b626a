// nmf.hip — non-negative matrix factorisation of the GF-ICF matrix, A ~ W diag(d) H, by alternating non-negative least
// squares.  Built into libgficf_nmf.so, which links libgficf_hip.so and uses its context, pool, transpose, scan and error
// plumbing; include/gficf_nmf.h states the method.
//
// Shared with pca.hip and svds.hip as text (pca_kernels.h): Y = A'X (k_pca_spmm), the chunked Gram matrix (k_pca_gram) and
// the chunked column sum (k_pca_colsum), with their layout: dense operands ROW-major with a pitch rounded up to 8, the Gram
// matrix with the pitch 16 .. 128.  Their explicit fma() calls stay fused under this file's -ffp-contract=off; everything
// written here rounds every product and every sum.
// Launches of one half-step (nm_half): k_pca_gram + k_pca_gram_fin, k_nmf_ridge; k_pca_spmm + k_pca_spmm_sum (k_nmf_sub
// with an L1 penalty); k_nmf_warm with a warm start; k_nmf_nnls, the solve; k_pca_colsum + k_pca_colsum_fin, k_nmf_dfin,
// k_nmf_norm.  Of an iteration: two half-steps, a copy of W between them, k_nmf_cor + k_nmf_cor_fin, then one read-back.
// Of the loss: k_nmf_sumsq, the product, k_nmf_cross, two Gram matrices, k_nmf_loss_fin.
// No floating-point atomic anywhere (the status word takes integer ORs, the count of capped rows integer adds).
#include <cmath>
#include <vector>

#include "addon_status.h"
#include "block_ops.h"
#include "common.h"
#include "gficf_nmf.h"
#include "pca_kernels.h"

namespace {

static_assert(GFICF_NMF_MAX_K == PCA_MAX_L, "the factors share the layout of pca_kernels.h");
constexpr uint32_t NMF_ST_NEG = 4u;        // a negative entry of A or of a start (beside PCA_ST_CSC, PCA_ST_VALUE)
constexpr int NMF_WG_WIDE = 1024;          // threads of the solve for k > 64: 16 rows at a time, S (up to 128 KiB) loaded once
constexpr int NMF_WG_NARROW = 256;         // for k <= 64: 4 rows at a time, S at most 32 KiB, several workgroups per CU
constexpr size_t NMF_HEAD = 16;            // int64 words behind the status word: dead / capped of either side, spare
enum { NC_DEAD_H, NC_CAP_H, NC_DEAD_W, NC_CAP_W, NC_DEAD, NC_CAP, NC_N };
// the scalars of an iteration, read back as one block
enum { NS_DELTA, NS_LOSS, NS_NORMA, NS_CROSS, NS_QUAD, NS_STATUS, NS_DEAD, NS_CAPPED, NS_N };

// ------------------------------------------------------------------------------------------------ the solve
__device__ inline double nmf_bcast(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

// One wave per row: lane l holds g, h and inv of the coordinates l and l + 64.  S sits in LDS transposed, sT[j k + l] =
// S[l][j], so that the update of g for coordinate j reads consecutive words; the values of coordinate j reach every lane by
// v_readlane, so D is uniform over the wave and `D != 0` is a uniform branch (the common case once a solution is sparse is
// the skip).  Nothing here is a sum over lanes.
template <int CPL, int T>
__global__ __launch_bounds__(T) void k_nmf_nnls(int64_t M, int k, int ld, const double* __restrict__ S, int lds, const double* __restrict__ B,
                                                const double* H0, double cd_tol, int cd_maxit, double* H, int32_t* __restrict__ sweeps,
                                                unsigned long long* __restrict__ capped) {
  extern __shared__ double nm_dyn[];
  double* const sT = nm_dyn;
  double* const sInv = nm_dyn + (size_t)k * k;
  for (int q = threadIdx.x; q < k * k; q += T) sT[q] = S[(size_t)(q % k) * lds + q / k];
  for (int j = threadIdx.x; j < k; j += T) {
    const double s = S[(size_t)j * lds + j];
    sInv[j] = s > 0.0 ? 1.0 / s : 0.0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  constexpr int NW = T / 64;
  for (int64_t r = (int64_t)blockIdx.x * NW + wv; r < M; r += (int64_t)gridDim.x * NW) {
    double g[CPL], h[CPL], iv[CPL];
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
      const int col = lane + cc * 64;
      const bool in = col < k;
      iv[cc] = in ? sInv[col] : 0.0;
      g[cc] = in ? -B[r * ld + col] : 0.0;
      h[cc] = (in && H0 && iv[cc] != 0.0) ? H0[r * ld + col] : 0.0;
    }
    if (H0) {
#pragma unroll
      for (int cj = 0; cj < CPL; ++cj) {
        const int nj = k - cj * 64 < 64 ? k - cj * 64 : 64;
        for (int jj = 0; jj < nj; ++jj) {
          const double hj = nmf_bcast(h[cj], jj);
          if (hj != 0.0) {
            const double* col = sT + (size_t)(cj * 64 + jj) * k;
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc)
              if (lane + cc * 64 < k) g[cc] = g[cc] + hj * col[lane + cc * 64];
          }
        }
      }
    }
    int sw = 0;
    bool met = false;
    while (sw < cd_maxit) {
      double meas = 0.0;
#pragma unroll
      for (int cj = 0; cj < CPL; ++cj) {
        const int nj = k - cj * 64 < 64 ? k - cj * 64 : 64;
        for (int jj = 0; jj < nj; ++jj) {
          const double invj = nmf_bcast(iv[cj], jj);
          if (invj == 0.0) continue;
          const double gj = nmf_bcast(g[cj], jj), hj = nmf_bcast(h[cj], jj);
          const double x = hj - gj * invj;
          const double hn = x > 0.0 ? x : 0.0, dl = hn - hj;
          if (dl != 0.0) {
            const double* col = sT + (size_t)(cj * 64 + jj) * k;
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc)
              if (lane + cc * 64 < k) g[cc] = g[cc] + dl * col[lane + cc * 64];
            if (lane == jj) h[cj] = hn;
            meas = fmax(meas, fabs(dl) / (hn + 1e-15));
          }
        }
      }
      ++sw;
      if (meas < cd_tol) { met = true; break; }
    }
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc)
      if (lane + cc * 64 < ld) H[r * ld + lane + cc * 64] = h[cc];
    if (lane == 0) {
      sweeps[r] = sw;
      if (!met && capped) atomicAdd(capped, 1ull);
    }
  }
}

int nm_nnls(gficf_ctx* ctx, int64_t M, int k, const double* S, int lds, const double* B, const double* H0, double cd_tol, int cd_maxit, double* H,
            int32_t* sweeps, unsigned long long* capped) {
  const size_t lds_bytes = ((size_t)k * k + k) * sizeof(double);
  const int ld = pca_ld(k);
  hipStream_t st = ctx->stream;
  if (k > 64) {
    GFICF_HIP_CHECK(hipFuncSetAttribute((const void*)k_nmf_nnls<2, NMF_WG_WIDE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)(((size_t)PCA_MAX_L * PCA_MAX_L + PCA_MAX_L) * sizeof(double))));
    const int64_t nb = gficf_ceil_div(M, NMF_WG_WIDE / 64), cap = ctx->num_cus;              // one workgroup per CU holds S
    hipLaunchKernelGGL((k_nmf_nnls<2, NMF_WG_WIDE>), dim3((unsigned)(nb < cap ? nb : cap)), dim3(NMF_WG_WIDE), lds_bytes, st, M, k, ld, S, lds, B, H0,
                       cd_tol, cd_maxit, H, sweeps, capped);
  } else {
    const int64_t nb = gficf_ceil_div(M, NMF_WG_NARROW / 64), cap = (int64_t)ctx->num_cus * 8;
    hipLaunchKernelGGL((k_nmf_nnls<1, NMF_WG_NARROW>), dim3((unsigned)(nb < cap ? nb : cap)), dim3(NMF_WG_NARROW), lds_bytes, st, M, k, ld, S, lds, B,
                       H0, cd_tol, cd_maxit, H, sweeps, capped);
  }
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// ------------------------------------------------------------------------------------------------ the small steps
// the first k columns of a dense operand looked at (finite, not negative) and, with out, copied with the padding zeroed
__global__ __launch_bounds__(256) void k_nmf_take(const double* in, int64_t rows, int k, int ld, double* out, uint32_t* __restrict__ status) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < rows * ld; q += (int64_t)gridDim.x * 256) {
    double v = 0.0;
    if ((int)(q % ld) < k) {
      v = in[q];
      if (!isfinite(v)) atomicOr(status, PCA_ST_VALUE);
      else if (v < 0.0) atomicOr(status, NMF_ST_NEG);
    }
    if (out) out[q] = v;
  }
}

__global__ __launch_bounds__(128) void k_nmf_ridge(double* __restrict__ S, int lp, int k, double ridge) {
  if ((int)threadIdx.x < k) S[threadIdx.x * lp + threadIdx.x] += ridge;
}

__global__ __launch_bounds__(256) void k_nmf_sub(double* __restrict__ B, int64_t n, double l1) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) B[q] = B[q] - l1;
}

__global__ __launch_bounds__(256) void k_nmf_warm(double* __restrict__ Y, int64_t rows, int k, int ld, const double* __restrict__ d) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < rows * ld; q += (int64_t)gridDim.x * 256) {
    const int j = (int)(q % ld);
    Y[q] = j < k ? Y[q] * d[j] : 0.0;
  }
}

// d[j] = the column sum; the dead factors counted
__global__ __launch_bounds__(PCA_MAX_L) void k_nmf_dfin(const double* __restrict__ cvec, int k, double* __restrict__ d, int64_t* __restrict__ dead) {
  const int j = threadIdx.x;
  const double s = j < k ? cvec[j] : 1.0;
  const int cnt = __syncthreads_count(!(s > 0.0));
  if (j < k) d[j] = s > 0.0 ? s : 0.0;
  if (j == 0) *dead = cnt;
}

__global__ __launch_bounds__(256) void k_nmf_norm(double* __restrict__ Y, int64_t rows, int k, int ld, const double* __restrict__ d) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < rows * ld; q += (int64_t)gridDim.x * 256) {
    const int j = (int)(q % ld);
    const double dd = j < k ? d[j] : 0.0;
    Y[q] = dd > 0.0 ? Y[q] / dd : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------ sums in fixed chunks
// part[b] = the sum of x^2 over chunk b of the stored entries; a negative or non-finite entry is flagged
__global__ __launch_bounds__(256) void k_nmf_sumsq(const double* __restrict__ x, int64_t nnz, int64_t per, double* __restrict__ part,
                                                   uint32_t* __restrict__ status) {
  __shared__ double s[256];
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < nnz ? lo + per : nnz;
  double acc = 0.0;
  for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
    const double v = x[p];
    if (!isfinite(v)) atomicOr(status, PCA_ST_VALUE);
    else if (v < 0.0) atomicOr(status, NMF_ST_NEG);
    acc = acc + v * v;
  }
  acc = gficf_block_sum_f64(acc, s);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// part[b] = sum over chunk b of the rows of sum_j (B[i][j] d[j]) H[i][j]
__global__ __launch_bounds__(256) void k_nmf_cross(const double* __restrict__ B, const double* __restrict__ H, const double* __restrict__ d, int64_t rows,
                                                   int k, int ld, int64_t rpc, double* __restrict__ part) {
  __shared__ double s[256];
  const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rpc, r1 = r0 + rpc < rows ? r0 + rpc : rows;
  double acc = 0.0;
  for (int64_t r = r0 + rl; r < r1; r += 4)
    for (int col = lane; col < k; col += 64) acc = acc + (B[r * ld + col] * d[col]) * H[r * ld + col];
  acc = gficf_block_sum_f64(acc, s);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// the chunks added in order, the quadratic term, the loss: out[0 .. 4) = loss, ||A||^2, cross, quad
__global__ __launch_bounds__(256) void k_nmf_loss_fin(const double* __restrict__ apart, int na, const double* __restrict__ cpart, int nc,
                                                      const double* __restrict__ S1, const double* __restrict__ S2, const double* __restrict__ d, int lp,
                                                      int k, double* __restrict__ out) {
  __shared__ double s[256];
  double acc = 0.0;
  for (int q = threadIdx.x; q < k * k; q += 256) {
    const int j = q / k, l = q % k;
    acc = acc + ((d[j] * S1[j * lp + l]) * d[l]) * S2[j * lp + l];
  }
  acc = gficf_block_sum_f64(acc, s);
  if (threadIdx.x == 0) {
    double a = 0.0, c = 0.0;
    for (int i = 0; i < na; ++i) a = a + apart[i];
    for (int i = 0; i < nc; ++i) c = c + cpart[i];
    out[0] = (a - 2.0 * c) + acc;
    out[1] = a;
    out[2] = c;
    out[3] = acc;
  }
}

// part[b][0 .. 5) = the sums of x, y, x^2, y^2, x y over chunk b of the rows (x = W, y = the previous W, the first k columns)
__global__ __launch_bounds__(256) void k_nmf_cor(const double* __restrict__ X, const double* __restrict__ Y, int64_t rows, int k, int ld, int64_t rpc,
                                                 double* __restrict__ part) {
  __shared__ double s[256];
  const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rpc, r1 = r0 + rpc < rows ? r0 + rpc : rows;
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t r = r0 + rl; r < r1; r += 4)
    for (int col = lane; col < k; col += 64) {
      const double x = X[r * ld + col], y = Y[r * ld + col];
      a[0] = a[0] + x; a[1] = a[1] + y; a[2] = a[2] + x * x; a[3] = a[3] + y * y; a[4] = a[4] + x * y;
    }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const double t = gficf_block_sum_f64(a[i], s);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * 5 + i] = t;
  }
}

// delta = 1 - cor, and the iteration's block of scalars completed: the status word and the counts as f64
__global__ void k_nmf_cor_fin(const double* __restrict__ part, int nch, double n, const uint32_t* __restrict__ status, const int64_t* __restrict__ counts,
                              double* __restrict__ scal) {
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int ch = 0; ch < nch; ++ch)
    for (int i = 0; i < 5; ++i) a[i] = a[i] + part[(int64_t)ch * 5 + i];
  const double vx = n * a[2] - a[0] * a[0], vy = n * a[3] - a[1] * a[1], cxy = n * a[4] - a[0] * a[1];
  scal[NS_DELTA] = (vx > 0.0 && vy > 0.0) ? 1.0 - cxy / sqrt(vx * vy) : 1.0;
  scal[NS_STATUS] = (double)*status;
  scal[NS_DEAD] = (double)counts[NC_DEAD_W];
  scal[NS_CAPPED] = (double)(counts[NC_CAP_H] + counts[NC_CAP_W]);
}

__global__ void k_nmf_counts_out(const int64_t* __restrict__ counts, int dead_at, int cap_at, int64_t* __restrict__ out) {
  out[0] = counts[dead_at];
  out[1] = counts[cap_at];
}

// ------------------------------------------------------------------------------------------------ workspace
struct NmWs {
  uint32_t* status;
  int64_t* counts;
  double* scal;
  void* tr_ws;
  size_t tr_bytes;
  int64_t* tptr;
  int32_t* tidx;
  double* tx;
  int64_t *segM, *segT;
  double *part, *B, *prev, *rpart, *apart, *gpart, *S, *S2, *cpart, *cvec;
  int32_t* sweeps;
};

size_t nm_carve(char* base, int64_t G, int64_t N, int64_t nnz, int k, NmWs& w) {
  gficf_carver cv;
  cv.base = base;
  const size_t n1 = (size_t)(nnz > 0 ? nnz : 1), nl = (size_t)(G < N ? N : G);
  const size_t ld = (size_t)pca_ld(k), lp2 = (size_t)pca_lp(k) * (size_t)pca_lp(k);
  w.status = cv.take<uint32_t>(1);
  w.counts = cv.take<int64_t>(NMF_HEAD);
  w.scal = cv.take<double>(NS_N);
  const size_t tr_a = gficf_csc_transpose_workspace_bytes(G, N), tr_b = gficf_csc_transpose_workspace_bytes(N, G);
  w.tr_bytes = tr_a > tr_b ? tr_a : tr_b;                    // (the size is the same for the matrix and for its transpose)
  w.tr_ws = cv.take<char>(w.tr_bytes);
  w.tptr = cv.take<int64_t>(nl + 1);
  w.tidx = cv.take<int32_t>(n1);
  w.tx = cv.take<double>(n1);
  w.segM = cv.take<int64_t>(nl + 1);
  w.segT = cv.take<int64_t>(nl + 1);
  w.part = cv.take<double>((size_t)pca_max_units((int64_t)nl, nnz) * ld);
  w.B = cv.take<double>(nl * ld);
  w.prev = cv.take<double>(nl * ld);
  w.rpart = cv.take<double>((size_t)PCA_CHUNKS * 5);
  w.apart = cv.take<double>((size_t)PCA_CHUNKS);
  w.gpart = cv.take<double>((size_t)pca_chunks((int64_t)nl) * lp2);
  w.S = cv.take<double>(lp2);
  w.S2 = cv.take<double>(lp2);
  w.cpart = cv.take<double>((size_t)PCA_CHUNKS * PCA_MAX_L);
  w.cvec = cv.take<double>(PCA_MAX_L);
  w.sweeps = cv.take<int32_t>(nl);
  return cv.total();
}

// what every entry on a matrix asks of its sizes
int nm_check(int64_t G, int64_t N, int64_t nnz, int k) {
  if (G < 1 || N < 1 || nnz < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "%lld x %lld, nnz = %lld: the matrix needs a row and a column", (long long)G, (long long)N, (long long)nnz);
  if (G > INT32_MAX || N > INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^31 - 1 rows or columns");
  if (k < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %d: at least one factor is required", k);
  if (k > GFICF_NMF_MAX_K) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "k = %d: at most %d factors", k, GFICF_NMF_MAX_K);
  return GFICF_OK;
}

int nm_check_cd(double ridge, double cd_tol, int cd_maxit) {
  if (!(ridge >= 0.0) || !(cd_tol >= 0.0) || cd_maxit < 0)
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ridge = %g, cd_tol = %g, cd_maxit = %d: none may be negative", ridge, cd_tol, cd_maxit);
  return GFICF_OK;
}

int nm_bind(int64_t G, int64_t N, int64_t nnz, int k, void* ws, size_t ws_bytes, NmWs& w) {
  if (!ws) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL workspace");
  return gficf_addon_carve(ws, ws_bytes, [&](char* base) { return nm_carve(base, G, N, nnz, k, w); });
}

// ------------------------------------------------------------------------------------------------ the stages
// S = Y'Y for the m x ld matrix Y: fixed chunks of rows, added in order
int nm_gram(gficf_ctx* ctx, const NmWs& w, const double* Y, int64_t m, int k, double* S) {
  const int ld = pca_ld(k), lp = pca_lp(k);
  const int64_t nch = pca_chunks(m), rpc = gficf_ceil_div(m, nch);
  const dim3 grid((unsigned)nch), blk(256);
  hipStream_t st = ctx->stream;
  if (lp == 16) hipLaunchKernelGGL(k_pca_gram<1>, grid, blk, 0, st, Y, m, ld, rpc, w.gpart);
  else if (lp == 32) hipLaunchKernelGGL(k_pca_gram<2>, grid, blk, 0, st, Y, m, ld, rpc, w.gpart);
  else if (lp == 64) hipLaunchKernelGGL(k_pca_gram<4>, grid, blk, 0, st, Y, m, ld, rpc, w.gpart);
  else hipLaunchKernelGGL(k_pca_gram<8>, grid, blk, 0, st, Y, m, ld, rpc, w.gpart);
  hipLaunchKernelGGL(k_pca_gram_fin, dim3(pca_grid(lp * lp)), blk, 0, st, (const double*)w.gpart, (int)nch, lp * lp, S);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// steps 1 - 3 on A (n_in rows, n_out columns, prepared): X (n_in x ld) -> Y (n_out x ld), d; dead / capped into counts
int nm_half(gficf_ctx* ctx, const NmWs& w, const PcaCsc& A, int k, const double* X, double* Y, double* d, int warm, double l1, double ridge,
            double cd_tol, int cd_maxit, int32_t* sweeps, int dead_at, int cap_at, bool normalise) {
  const int ld = pca_ld(k), lp = pca_lp(k);
  const int64_t n_in = A.nrows, n_out = A.ncols;
  hipStream_t st = ctx->stream;
  GFICF_RC(nm_gram(ctx, w, X, n_in, k, w.S));
  hipLaunchKernelGGL(k_nmf_ridge, dim3(1), dim3(128), 0, st, w.S, lp, k, ridge);
  GFICF_HIP_CHECK(hipGetLastError());
  GFICF_RC(pca_spmm(ctx, A, X, k, w.B, w.part, w.status));
  if (l1 != 0.0) hipLaunchKernelGGL(k_nmf_sub, dim3(pca_grid(n_out * ld)), dim3(256), 0, st, w.B, n_out * ld, l1);
  if (warm) hipLaunchKernelGGL(k_nmf_warm, dim3(pca_grid(n_out * ld)), dim3(256), 0, st, Y, n_out, k, ld, (const double*)d);
  GFICF_HIP_CHECK(hipGetLastError());
  GFICF_HIP_CHECK(hipMemsetAsync(w.counts + cap_at, 0, sizeof(int64_t), st));
  GFICF_RC(nm_nnls(ctx, n_out, k, w.S, lp, w.B, warm ? Y : nullptr, cd_tol, cd_maxit, Y, sweeps, (unsigned long long*)(w.counts + cap_at)));
  if (!normalise) return GFICF_OK;
  const int64_t nch = pca_chunks(n_out), rpc = gficf_ceil_div(n_out, nch);
  hipLaunchKernelGGL(k_pca_colsum, dim3((unsigned)nch), dim3(256), 0, st, (const double*)Y, n_out, ld, (const double*)nullptr, rpc, w.cpart);
  hipLaunchKernelGGL(k_pca_colsum_fin, dim3(1), dim3(PCA_MAX_L), 0, st, (const double*)w.cpart, (int)nch, w.cvec);
  hipLaunchKernelGGL(k_nmf_dfin, dim3(1), dim3(PCA_MAX_L), 0, st, (const double*)w.cvec, k, d, w.counts + dead_at);
  hipLaunchKernelGGL(k_nmf_norm, dim3(pca_grid(n_out * ld)), dim3(256), 0, st, Y, n_out, k, ld, (const double*)d);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// w.apart[0 .. na) = the chunks of ||A||^2; A's entries looked at
int nm_sumsq(gficf_ctx* ctx, const NmWs& w, const double* x, int64_t nnz, int* na) {
  const int64_t nch = pca_chunks(nnz), per = gficf_ceil_div(nnz > 0 ? nnz : 1, nch);
  hipLaunchKernelGGL(k_nmf_sumsq, dim3((unsigned)nch), dim3(256), 0, ctx->stream, x, nnz, per, w.apart, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  *na = (int)nch;
  return GFICF_OK;
}

// out[0 .. 4) from the chunks of ||A||^2, A (G x N, prepared), W, d, H
int nm_loss(gficf_ctx* ctx, const NmWs& w, const PcaCsc& A, int na, int k, const double* W, const double* d, const double* H, double* out) {
  const int ld = pca_ld(k), lp = pca_lp(k);
  const int64_t G = A.nrows, N = A.ncols;
  hipStream_t st = ctx->stream;
  GFICF_RC(pca_spmm(ctx, A, W, k, w.B, w.part, w.status));
  const int64_t nch = pca_chunks(N), rpc = gficf_ceil_div(N, nch);
  hipLaunchKernelGGL(k_nmf_cross, dim3((unsigned)nch), dim3(256), 0, st, (const double*)w.B, H, d, N, k, ld, rpc, w.rpart);
  GFICF_HIP_CHECK(hipGetLastError());
  GFICF_RC(nm_gram(ctx, w, W, G, k, w.S));
  GFICF_RC(nm_gram(ctx, w, H, N, k, w.S2));
  hipLaunchKernelGGL(k_nmf_loss_fin, dim3(1), dim3(256), 0, st, (const double*)w.apart, na, (const double*)w.rpart, (int)nch, (const double*)w.S,
                     (const double*)w.S2, d, lp, k, out);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int nm_take(gficf_ctx* ctx, const NmWs& w, const double* in, int64_t rows, int k, double* out) {
  hipLaunchKernelGGL(k_nmf_take, dim3(pca_grid(rows * pca_ld(k))), dim3(256), 0, ctx->stream, in, rows, k, pca_ld(k), out, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int nm_copy_out(gficf_ctx* ctx, const NmWs& w, int64_t n_out, int k, double* d_S, double* d_B, int32_t* d_sweeps) {
  const size_t lp = (size_t)pca_lp(k);
  if (d_S) GFICF_HIP_CHECK(hipMemcpyAsync(d_S, w.S, sizeof(double) * lp * lp, hipMemcpyDeviceToDevice, ctx->stream));
  if (d_B) GFICF_HIP_CHECK(hipMemcpyAsync(d_B, w.B, sizeof(double) * (size_t)n_out * (size_t)pca_ld(k), hipMemcpyDeviceToDevice, ctx->stream));
  if (d_sweeps) GFICF_HIP_CHECK(hipMemcpyAsync(d_sweeps, w.sweeps, sizeof(int32_t) * (size_t)n_out, hipMemcpyDeviceToDevice, ctx->stream));
  return GFICF_OK;
}

// row-major rows x k without padding <-> rows x ld on the device
hipError_t nm_up(gficf_ctx* ctx, double* dst, const double* src, int64_t rows, int k) {
  const size_t ld = (size_t)pca_ld(k);
  hipError_t e = hipMemsetAsync(dst, 0, sizeof(double) * (size_t)rows * ld, ctx->stream);
  if (e == hipSuccess) e = hipMemcpy2DAsync(dst, ld * sizeof(double), src, (size_t)k * sizeof(double), (size_t)k * sizeof(double), (size_t)rows, hipMemcpyHostToDevice, ctx->stream);
  return e;
}
hipError_t nm_down(gficf_ctx* ctx, double* dst, const double* src, int64_t rows, int k) {
  return hipMemcpy2DAsync(dst, (size_t)k * sizeof(double), src, (size_t)pca_ld(k) * sizeof(double), (size_t)k * sizeof(double), (size_t)rows, hipMemcpyDeviceToHost,
                          ctx->stream);
}

}  // namespace

extern "C" {

int gficf_nmf_abi_version(void) { return GFICF_NMF_ABI_VERSION; }

size_t gficf_nmf_workspace_bytes(int64_t G, int64_t N, int64_t nnz, int k) {
  if (G < 1 || N < 1 || nnz < 0 || G > INT32_MAX || N > INT32_MAX || k < 1 || k > GFICF_NMF_MAX_K) return 0;
  NmWs w;
  return nm_carve(nullptr, G, N, nnz, k, w);
}

int gficf_nnls_device(gficf_ctx* ctx, int64_t M, int k, const double* d_S, int ld_s, const double* d_B, const double* d_H0, double cd_tol,
                      int cd_maxit, double* d_H, int32_t* d_sweeps, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(nm_check(M, M, 0, k));
  GFICF_RC(nm_check_cd(0.0, cd_tol, cd_maxit));
  if (ld_s < k) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ld_s = %d: the pitch of S must be at least k = %d", ld_s, k);
  if (!d_S || !d_B || !d_H || !d_sweeps || !ws) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (ws_bytes < GFICF_NMF_NNLS_WS_BYTES) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "workspace too small: %zu < %d bytes", ws_bytes, GFICF_NMF_NNLS_WS_BYTES);
  return nm_nnls(ctx, M, k, d_S, ld_s, d_B, d_H0, cd_tol, cd_maxit, d_H, d_sweeps, nullptr);
}

int gficf_nmf_half_device(gficf_ctx* ctx, int64_t n_in, int64_t n_out, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x,
                          int64_t nnz, int k, const double* d_X, double* d_Y, double* d_d, int warm, double l1, double ridge, double cd_tol,
                          int cd_maxit, double* d_S, double* d_B, int32_t* d_sweeps, int64_t* d_counts, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(nm_check(n_in, n_out, nnz, k));
  GFICF_RC(nm_check_cd(ridge, cd_tol, cd_maxit));
  if (!(l1 >= 0.0)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "l1 = %g: the penalty may not be negative", l1);
  if (!d_colptr || !d_X || !d_Y || !d_d || (nnz > 0 && (!d_rowidx || !d_x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  NmWs w;
  GFICF_RC(nm_bind(n_in, n_out, nnz, k, ws, ws_bytes, w));
  const PcaCsc A{n_in, n_out, nnz, d_colptr, d_rowidx, d_x, w.segM, pca_max_units(n_out, nnz)};
  int na;
  GFICF_RC(pca_csc_prepare(ctx, A, w.status));
  GFICF_RC(nm_sumsq(ctx, w, d_x, nnz, &na));
  GFICF_RC(nm_take(ctx, w, d_X, n_in, k, nullptr));
  if (warm) GFICF_RC(nm_take(ctx, w, d_Y, n_out, k, nullptr));
  GFICF_RC(nm_half(ctx, w, A, k, d_X, d_Y, d_d, warm, l1, ridge, cd_tol, cd_maxit, w.sweeps, NC_DEAD, NC_CAP, true));
  if (d_counts) {
    hipLaunchKernelGGL(k_nmf_counts_out, dim3(1), dim3(1), 0, ctx->stream, (const int64_t*)w.counts, (int)NC_DEAD, (int)NC_CAP, d_counts);
    GFICF_HIP_CHECK(hipGetLastError());
  }
  return nm_copy_out(ctx, w, n_out, k, d_S, d_B, d_sweeps);
}

int gficf_nmf_loss_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int64_t nnz,
                          int k, const double* d_W, const double* d_d, const double* d_H, double* d_loss, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(nm_check(G, N, nnz, k));
  if (!d_colptr || !d_W || !d_d || !d_H || !d_loss || (nnz > 0 && (!d_rowidx || !d_x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  NmWs w;
  GFICF_RC(nm_bind(G, N, nnz, k, ws, ws_bytes, w));
  const PcaCsc A{G, N, nnz, d_colptr, d_rowidx, d_x, w.segM, pca_max_units(N, nnz)};
  int na;
  GFICF_RC(pca_csc_prepare(ctx, A, w.status));
  GFICF_RC(nm_sumsq(ctx, w, d_x, nnz, &na));
  return nm_loss(ctx, w, A, na, k, d_W, d_d, d_H, d_loss);
}

int gficf_nmf_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int64_t nnz,
                     int k, const double* d_W0, double tol, int maxit, double l1_w, double l1_h, double ridge, double cd_tol, int cd_maxit,
                     int track_loss, double* d_W, double* d_d, double* d_H, double* h_delta, double* h_loss, int64_t* h_info, void* ws,
                     size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(nm_check(G, N, nnz, k));
  if (k > (G < N ? G : N)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %d: at most min(G, N) = %lld factors", k, (long long)(G < N ? G : N));
  GFICF_RC(nm_check_cd(ridge, cd_tol, cd_maxit));
  if (!(tol >= 0.0) || maxit < 0 || !(l1_w >= 0.0) || !(l1_h >= 0.0))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "tol = %g, maxit = %d, L1 = (%g, %g): none may be negative", tol, maxit, l1_w, l1_h);
  if (!d_colptr || !d_W0 || !d_W || !d_d || !d_H || !h_info || (maxit > 0 && !h_delta) || (track_loss && maxit > 0 && !h_loss) ||
      (nnz > 0 && (!d_rowidx || !d_x)))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  NmWs w;
  GFICF_RC(nm_bind(G, N, nnz, k, ws, ws_bytes, w));
  const int ld = pca_ld(k);
  hipStream_t st = ctx->stream;
  GFICF_HIP_CHECK(hipMemsetAsync(w.counts, 0, sizeof(int64_t) * NMF_HEAD, st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.scal, 0, sizeof(double) * NS_N, st));
  GFICF_HIP_CHECK(hipMemsetAsync(d_d, 0, sizeof(double) * (size_t)k, st));
  GFICF_HIP_CHECK(hipMemsetAsync(d_H, 0, sizeof(double) * (size_t)N * (size_t)ld, st));
  // the gene-major view: M (genes x cells CSC) gives A'X, its transpose T gives A X
  GFICF_RC(gficf_csc_transpose_device(ctx, G, N, d_colptr, d_rowidx, d_x, nnz, w.tptr, w.tidx, w.tx, w.tr_ws, w.tr_bytes));
  const PcaCsc M{G, N, nnz, d_colptr, d_rowidx, d_x, w.segM, pca_max_units(N, nnz)};
  const PcaCsc T{N, G, nnz, w.tptr, w.tidx, w.tx, w.segT, pca_max_units(G, nnz)};
  GFICF_RC(pca_csc_prepare(ctx, M, w.status));
  GFICF_RC(pca_csc_prepare(ctx, T, w.status));
  int na;
  GFICF_RC(nm_sumsq(ctx, w, d_x, nnz, &na));
  GFICF_RC(nm_take(ctx, w, d_W0, G, k, d_W));
  const int64_t nch = pca_chunks(G), rpc = gficf_ceil_div(G, nch);
  double scal[NS_N] = {0.0};
  int it = 0, stopped = 0;
  while (it < maxit) {
    GFICF_RC(nm_half(ctx, w, M, k, d_W, d_H, d_d, it > 0, l1_h, ridge, cd_tol, cd_maxit, w.sweeps, NC_DEAD_H, NC_CAP_H, true));
    GFICF_HIP_CHECK(hipMemcpyAsync(w.prev, d_W, sizeof(double) * (size_t)G * (size_t)ld, hipMemcpyDeviceToDevice, st));
    GFICF_RC(nm_half(ctx, w, T, k, d_H, d_W, d_d, 1, l1_w, ridge, cd_tol, cd_maxit, w.sweeps, NC_DEAD_W, NC_CAP_W, true));
    if (track_loss) GFICF_RC(nm_loss(ctx, w, M, na, k, d_W, d_d, d_H, w.scal + NS_LOSS));
    hipLaunchKernelGGL(k_nmf_cor, dim3((unsigned)nch), dim3(256), 0, st, (const double*)d_W, (const double*)w.prev, G, k, ld, rpc, w.rpart);
    hipLaunchKernelGGL(k_nmf_cor_fin, dim3(1), dim3(1), 0, st, (const double*)w.rpart, (int)nch, (double)G * (double)k, (const uint32_t*)w.status,
                       (const int64_t*)w.counts, w.scal);
    GFICF_HIP_CHECK(hipGetLastError());
    GFICF_HIP_CHECK(hipMemcpyAsync(scal, w.scal, sizeof(double) * NS_N, hipMemcpyDeviceToHost, st));
    GFICF_HIP_CHECK(hipStreamSynchronize(st));
    h_delta[it] = scal[NS_DELTA];
    if (track_loss) h_loss[it] = scal[NS_LOSS];
    ++it;
    if (scal[NS_STATUS] != 0.0) break;
    if (scal[NS_DELTA] < tol) { stopped = 1; break; }
  }
  h_info[0] = it;
  h_info[1] = stopped;
  h_info[2] = (int64_t)scal[NS_DEAD];
  h_info[3] = (int64_t)scal[NS_CAPPED];
  return GFICF_OK;
}

int gficf_nmf_project_device(gficf_ctx* ctx, int64_t G, int64_t n_new, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x,
                             int64_t nnz, int k, const double* d_W, double ridge, double cd_tol, int cd_maxit, double* d_H, double* d_S,
                             double* d_B, int32_t* d_sweeps, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(nm_check(G, n_new, nnz, k));
  GFICF_RC(nm_check_cd(ridge, cd_tol, cd_maxit));
  if (!d_colptr || !d_W || !d_H || (nnz > 0 && (!d_rowidx || !d_x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  NmWs w;
  GFICF_RC(nm_bind(G, n_new, nnz, k, ws, ws_bytes, w));
  const PcaCsc A{G, n_new, nnz, d_colptr, d_rowidx, d_x, w.segM, pca_max_units(n_new, nnz)};
  int na;
  GFICF_RC(pca_csc_prepare(ctx, A, w.status));
  GFICF_RC(nm_sumsq(ctx, w, d_x, nnz, &na));
  GFICF_RC(nm_take(ctx, w, d_W, G, k, nullptr));
  GFICF_RC(nm_half(ctx, w, A, k, d_W, d_H, nullptr, 0, 0.0, ridge, cd_tol, cd_maxit, w.sweeps, NC_DEAD, NC_CAP, false));
  return nm_copy_out(ctx, w, n_new, k, d_S, d_B, d_sweeps);
}

int gficf_nmf_sync(gficf_ctx* ctx, void* ws) {
  uint32_t st;
  const int rc = gficf_addon_read_status(ctx, ws, &st);
  if (rc) return rc;
  if (st) {
    GFICF_HIP_CHECK(hipMemsetAsync(ws, 0, sizeof(uint32_t), ctx->stream));
    GFICF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  if (st & PCA_ST_CSC) GFICF_FAIL(GFICF_ERR_BAD_CSC, "a row index out of range or a bad column pointer");
  if (st & PCA_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "a NaN or an infinite value in the matrix or in a factor");
  if (st & NMF_ST_NEG) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "a negative entry in the matrix or in a start: the factorisation is of non-negative data");
  return GFICF_OK;
}

int gficf_nmf_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x, int k,
                   const double* W0, double tol, int maxit, double l1_w, double l1_h, double ridge, double cd_tol, int cd_maxit, int track_loss,
                   double* w, double* d, double* h, double* delta, double* loss, int64_t* info) {
  GFICF_CTX_ENTER(ctx);
  if (G < 1 || N < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld: the matrix needs a row and a column", (long long)G, (long long)N);
  if (!colptr || !W0 || !w || !d || !h || !info) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> cp;
  int64_t nnz = 0;
  GFICF_RC(gficf_host_colptr(colptr, colptr_is_i64, N, "colptr", cp, &nnz));
  GFICF_RC(nm_check(G, N, nnz, k));
  if (nnz > 0 && (!rowidx || !x)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t nsz = (size_t)(nnz > 0 ? nnz : 1), ld = (size_t)pca_ld(k);
  const size_t wsb = gficf_nmf_workspace_bytes(G, N, nnz, k);
  gficf_host_io io{ctx, "gficf_nmf_host"};
  gficf_carver cv;
  int64_t* d_cp; int32_t* d_ri; double *d_x, *d_W, *d_dd, *d_H; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_cp = cv.take<int64_t>((size_t)N + 1); d_ri = cv.take<int32_t>(nsz); d_x = cv.take<double>(nsz);
    d_W = cv.take<double>((size_t)G * ld); d_dd = cv.take<double>((size_t)k); d_H = cv.take<double>((size_t)N * ld);
    d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_cp, cp.data(), sizeof(int64_t) * cp.size());
  io.up(d_ri, rowidx, sizeof(int32_t) * (size_t)nnz);
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  if (io.ok()) io.e = nm_up(ctx, d_W, W0, G, k);
  if (io.ok()) io.e = hipMemsetAsync(d_ws, 0, sizeof(uint32_t), ctx->stream);
  int rc = GFICF_OK;
  if (io.ok()) {
    rc = gficf_nmf_device(ctx, G, N, d_cp, d_ri, d_x, nnz, k, d_W, tol, maxit, l1_w, l1_h, ridge, cd_tol, cd_maxit, track_loss, d_W, d_dd, d_H, delta,
                          loss, info, d_ws, wsb);
    if (!rc) {
      io.e = nm_down(ctx, w, d_W, G, k);
      if (io.ok()) io.e = nm_down(ctx, h, d_H, N, k);
      io.down(d, d_dd, sizeof(double) * (size_t)k);
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_nmf_sync(ctx, d_ws);
}

int gficf_nmf_project_host(gficf_ctx* ctx, int64_t G, int64_t n_new, const void* colptr, int colptr_is_i64, const int32_t* rowidx,
                           const double* x, int k, const double* w, double ridge, double cd_tol, int cd_maxit, double* h, int32_t* sweeps) {
  GFICF_CTX_ENTER(ctx);
  if (G < 1 || n_new < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, n_new = %lld: the matrix needs a row and a column", (long long)G, (long long)n_new);
  if (!colptr || !w || !h) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> cp;
  int64_t nnz = 0;
  GFICF_RC(gficf_host_colptr(colptr, colptr_is_i64, n_new, "colptr", cp, &nnz));
  GFICF_RC(nm_check(G, n_new, nnz, k));
  if (nnz > 0 && (!rowidx || !x)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t nsz = (size_t)(nnz > 0 ? nnz : 1), ld = (size_t)pca_ld(k);
  const size_t wsb = gficf_nmf_workspace_bytes(G, n_new, nnz, k);
  gficf_host_io io{ctx, "gficf_nmf_project_host"};
  gficf_carver cv;
  int64_t* d_cp; int32_t *d_ri, *d_sw; double *d_x, *d_W, *d_H; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_cp = cv.take<int64_t>((size_t)n_new + 1); d_ri = cv.take<int32_t>(nsz); d_x = cv.take<double>(nsz);
    d_W = cv.take<double>((size_t)G * ld); d_H = cv.take<double>((size_t)n_new * ld); d_sw = cv.take<int32_t>((size_t)n_new);
    d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_cp, cp.data(), sizeof(int64_t) * cp.size());
  io.up(d_ri, rowidx, sizeof(int32_t) * (size_t)nnz);
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  if (io.ok()) io.e = nm_up(ctx, d_W, w, G, k);
  if (io.ok()) io.e = hipMemsetAsync(d_ws, 0, sizeof(uint32_t), ctx->stream);
  int rc = GFICF_OK;
  if (io.ok()) {
    rc = gficf_nmf_project_device(ctx, G, n_new, d_cp, d_ri, d_x, nnz, k, d_W, ridge, cd_tol, cd_maxit, d_H, nullptr, nullptr, d_sw, d_ws, wsb);
    if (!rc) {
      io.e = nm_down(ctx, h, d_H, n_new, k);
      if (sweeps) io.down(sweeps, d_sw, sizeof(int32_t) * (size_t)n_new);
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_nmf_sync(ctx, d_ws);
}

}  // extern "C"
