// svds.hip — the exact truncated SVD behind randomized = FALSE of runPCA / runLSA / computePCADim (reference
// R/dimensinalityReduction.R:57,124,213,216: RSpectra::svds, rsvd::rpca(rand = FALSE)): block Lanczos with full
// reorthogonalisation, Rayleigh-Ritz and thick restart on C = At'At or At At'.  Built into libgficf_svds.so, which links
// libgficf_hip.so and uses its context, pool, transpose, scan and error plumbing; include/gficf_svds.h states the method.
//
// Shared with pca.hip as text (pca_kernels.h): Y = A'X at l = b (k_pca_spmm), the rank-one centring, the Gram matrix, the
// one-workgroup eigen-solve (the blocks' orth and the Ritz step), Y <- Y M, the sign rule and the layout conversion, with
// their layout: dense operands ROW-major with a pitch rounded up to 8, the small matrices with the pitch 16 .. 128.
// The Krylov machinery is this file's.  The widths of the blocks, the basis' column count and the kept count live in a
// state block ON THE DEVICE (a block narrows when orth drops directions, which the host does not wait to learn): the host
// enqueues every cycle's steps at full width, and a step whose cycle has ended does nothing.  Launches of one step:
//   k_svds_begin      the state of the step: where the block goes, the basis' new column count
//   k_svds_append     V[:, j0 .. j0 + bw) = Q
//   (k_pca_spmm twice, k_pca_colsum / k_pca_rank1 with centring)   W = C Q
//   k_svds_colss, k_svds_sigma   the columns' sums of squares over fixed chunks of rows; sigma = max(sigma, largest norm)
//   k_svds_proj(+_fin) P = V'W: up to 128 x 32 inner products over fixed chunks of rows, the chunks added in order
//   k_svds_hfill      P into H, both triangles
//   k_svds_update     W -= V P (and R = W behind the second pass)
//   k_svds_step_end   does the cycle end here
//   (k_pca_gram / k_pca_eig / k_pca_apply twice) with k_svds_trim   Qn = orth(W), the directions below tau * sigma dropped
//   k_svds_width, k_svds_copyq   the new block's width; Q = Qn
// of a cycle's end: k_pca_eig on H; k_svds_resid(+_fin): rho_i = ||R Z[last rows, i]||, the flags, the info block;
// of a restart: k_svds_restart_state, k_svds_rotate (V2 = V Z[:, :nk]), k_svds_restart_h, the projection and orth of R;
// of the finish: k_svds_rotate, k_pca_gram + k_svds_polish + k_pca_apply (one Newton-Schulz step on V_k), Y = A'X at l = k, k_svds_colss + k_svds_dfin (d), k_svds_colscale, k_pca_sign, k_pca_out.
// No floating-point atomic anywhere (the status word takes integer ORs): the same input gives the same bits on every call.
#include <cmath>
#include <vector>

#include "addon_status.h"
#include "common.h"
#include "gficf_svds.h"
#include "pca_kernels.h"

namespace {

constexpr int SV_MAXB = GFICF_SVDS_MAX_B;
constexpr int SV_MAXM = GFICF_SVDS_MAX_M;
constexpr int SV_PN = SV_MAXM * SV_MAXB;   // entries of P
static_assert(SV_MAXM == PCA_MAX_L, "the Ritz step is one k_pca_eig");

// the state block (int32)
enum { ST_COLS, ST_BW, ST_J0, ST_BWL, ST_ENDED, ST_EXH, ST_ACT, ST_ME, ST_NK, ST_PROD, ST_COPY, ST_N };

// ------------------------------------------------------------------------------------------------ the state of a step
__global__ void k_svds_begin(int* __restrict__ st, int m) {
  st[ST_ACT] = 0;
  if (st[ST_ENDED]) return;
  const int cols = st[ST_COLS], bw = st[ST_BW];
  if (bw < 1 || cols + bw > m) { st[ST_ENDED] = 1; return; }      // (the rules below never let a block not fit)
  st[ST_J0] = cols;
  st[ST_BWL] = bw;
  st[ST_COLS] = cols + bw;
  st[ST_PROD] += 1;
  st[ST_ACT] = 1;
}

__global__ void k_svds_step_end(int* __restrict__ st, int64_t n, int b, int m, int last) {
  if (!st[ST_ACT]) return;
  const int64_t cols = st[ST_COLS];
  const int64_t next = n - cols < b ? n - cols : b;
  if (cols >= n || cols + next > m || last) {
    st[ST_ENDED] = 1;
    if (cols >= n) st[ST_EXH] = 1;
  }
}

// the width of the block orth has left in Qn: the directions its second pass kept (they come first)
__global__ void k_svds_width(const double* __restrict__ dv, int b, int64_t n, int* __restrict__ st, int first) {
  st[ST_COPY] = 0;
  if (!first && (!st[ST_ACT] || st[ST_ENDED])) return;
  int w = 0;
  for (int j = 0; j < b; ++j) w += dv[j] > 0.0 ? 1 : 0;
  const int64_t room = n - st[ST_COLS];
  if (w > room) w = (int)(room > 0 ? room : 0);
  st[ST_BW] = w;
  st[ST_COPY] = 1;
  if (w == 0) { st[ST_ENDED] = 1; st[ST_EXH] = 1; }
}

__global__ __launch_bounds__(256) void k_svds_copyq(const double* __restrict__ Qn, double* __restrict__ Q, int64_t n, int ldb, const int* __restrict__ st) {
  if (!st[ST_COPY]) return;
  const int bw = st[ST_BW];
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n * ldb; q += (int64_t)gridDim.x * 256) Q[q] = (int)(q % ldb) < bw ? Qn[q] : 0.0;
}

__global__ __launch_bounds__(256) void k_svds_append(const double* __restrict__ Q, int ldb, double* __restrict__ V, int pv, int64_t n,
                                                     const int* __restrict__ st) {
  if (!st[ST_ACT]) return;
  const int j0 = st[ST_J0], bwl = st[ST_BWL];                  // j0 + bwl = |V| <= m <= pv
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n * ldb; q += (int64_t)gridDim.x * 256) {
    const int j = (int)(q % ldb);
    if (j < bwl) V[(q / ldb) * pv + j0 + j] = Q[q];
  }
}

// ------------------------------------------------------------------------------------------------ column norms
// part[chunk][col] = the sum of X[r][col]^2 over the chunk's rows (ld <= 128)
__global__ __launch_bounds__(256) void k_svds_colss(const double* __restrict__ X, int64_t rows, int ld, int64_t rpc, double* __restrict__ part) {
  __shared__ double s[4][SV_MAXM];
  const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rpc, r1 = r0 + rpc < rows ? r0 + rpc : rows;
  double acc[2] = {0.0, 0.0};
  for (int64_t r = r0 + rl; r < r1; r += 4)
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
      if (lane + cc * 64 < ld) {
        const double v = X[r * ld + lane + cc * 64];
        acc[cc] = fma(v, v, acc[cc]);
      }
  s[rl][lane] = acc[0];
  s[rl][lane + 64] = acc[1];
  __syncthreads();
  if (rl == 0)
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int col = lane + cc * 64;
      part[(int64_t)blockIdx.x * SV_MAXM + col] = ((s[0][col] + s[1][col]) + s[2][col]) + s[3][col];
    }
}

// sigma = max(sigma, the largest of the ncol column norms)
__global__ __launch_bounds__(SV_MAXM) void k_svds_sigma(const double* __restrict__ part, int nch, int ncol, const int* __restrict__ st, double* __restrict__ ds) {
  __shared__ double sN[SV_MAXM];
  if (!st[ST_ACT]) return;
  double s = 0.0;
  for (int ch = 0; ch < nch; ++ch) s += part[(int64_t)ch * SV_MAXM + threadIdx.x];
  sN[threadIdx.x] = sqrt(s);
  __syncthreads();
  if (threadIdx.x == 0) {
    double mx = ds[0];
    for (int j = 0; j < ncol; ++j) mx = fmax(mx, sN[j]);
    ds[0] = mx;
  }
}

// d[i] = the norm of column i, i < k
__global__ __launch_bounds__(SV_MAXM) void k_svds_dfin(const double* __restrict__ part, int nch, int k, double* __restrict__ d) {
  double s = 0.0;
  for (int ch = 0; ch < nch; ++ch) s += part[(int64_t)ch * SV_MAXM + threadIdx.x];
  if ((int)threadIdx.x < k) d[threadIdx.x] = sqrt(s);
}

// X[:, i] *= d[i] or, with inv, /= d[i] (a zero column where d[i] is 0), i < k
__global__ __launch_bounds__(256) void k_svds_colscale(double* __restrict__ X, int64_t rows, int ld, int k, const double* __restrict__ d, int inv) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < rows * ld; q += (int64_t)gridDim.x * 256) {
    const int j = (int)(q % ld);
    if (j >= k) continue;
    const double dd = d[j];
    X[q] = inv ? (dd > 0.0 ? X[q] / dd : 0.0) : X[q] * dd;
  }
}

// ------------------------------------------------------------------------------------------------ P = V'W, W -= V P
// one workgroup per chunk of rows; thread (tx, ty) of 32 x 8 holds P[ty + 8 a][tx], a < 16; rows staged 16 at a time
__global__ __launch_bounds__(256) void k_svds_proj(const double* __restrict__ V, int pv, const double* __restrict__ W, int ldb, int64_t n, int64_t rpc,
                                                   const int* __restrict__ st, double* __restrict__ part) {
  __shared__ double sV[16][SV_MAXM];
  __shared__ double sW[16][SV_MAXB];
  if (!st[ST_ACT]) return;
  const int cols = st[ST_COLS];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t r0 = (int64_t)blockIdx.x * rpc, r1 = r0 + rpc < n ? r0 + rpc : n;
  double acc[16];
#pragma unroll
  for (int a = 0; a < 16; ++a) acc[a] = 0.0;
  for (int64_t t0 = r0; t0 < r1; t0 += 16) {
    for (int q = threadIdx.x; q < 16 * SV_MAXM; q += 256) {
      const int rr = q / SV_MAXM, cc = q % SV_MAXM;
      sV[rr][cc] = (t0 + rr < r1 && cc < cols) ? V[(t0 + rr) * pv + cc] : 0.0;
    }
    for (int q = threadIdx.x; q < 16 * SV_MAXB; q += 256) {
      const int rr = q / SV_MAXB, cc = q % SV_MAXB;
      sW[rr][cc] = (t0 + rr < r1 && cc < ldb) ? W[(t0 + rr) * ldb + cc] : 0.0;
    }
    __syncthreads();
    for (int rr = 0; rr < 16; ++rr) {
      const double w = sW[rr][tx];
#pragma unroll
      for (int a = 0; a < 16; ++a)
        if (a * 8 < cols) acc[a] = fma(sV[rr][ty + 8 * a], w, acc[a]);
    }
    __syncthreads();
  }
  double* dst = part + (int64_t)blockIdx.x * SV_PN;
#pragma unroll
  for (int a = 0; a < 16; ++a) dst[(ty + 8 * a) * SV_MAXB + tx] = acc[a];
}

__global__ __launch_bounds__(256) void k_svds_proj_fin(const double* __restrict__ part, int nch, const int* __restrict__ st, double* __restrict__ P) {
  if (!st[ST_ACT]) return;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < SV_PN; q += gridDim.x * 256) {
    double s = 0.0;
    for (int ch = 0; ch < nch; ++ch) s += part[(int64_t)ch * SV_PN + q];
    P[q] = s;
  }
}

// H[:|V|, j0 .. j0 + bw) = P and its mirror image; the block's own corner symmetrised
__global__ __launch_bounds__(256) void k_svds_hfill(const double* __restrict__ P, double* __restrict__ H, int lp, const int* __restrict__ st) {
  if (!st[ST_ACT]) return;
  const int cols = st[ST_COLS], j0 = st[ST_J0], bwl = st[ST_BWL];
  for (int q = threadIdx.x; q < SV_PN; q += 256) {
    const int i = q / SV_MAXB, j = q % SV_MAXB;
    if (i >= cols || j >= bwl) continue;
    if (i < j0) {
      H[i * lp + j0 + j] = P[q];
      H[(j0 + j) * lp + i] = P[q];
    } else {
      H[i * lp + j0 + j] = 0.5 * (P[q] + P[(j0 + j) * SV_MAXB + (i - j0)]);
    }
  }
}

// W[r][j] -= sum over i < |V| of V[r][i] P[i][j], in that order; R (if given) receives the result as well
__global__ __launch_bounds__(256) void k_svds_update(const double* __restrict__ V, int pv, const double* __restrict__ P, double* __restrict__ W, int ldb,
                                                     int64_t n, const int* __restrict__ st, double* __restrict__ R) {
  __shared__ double sP[SV_PN];
  if (!st[ST_ACT]) return;
  const int cols = st[ST_COLS];
  for (int q = threadIdx.x; q < SV_PN; q += 256) sP[q] = P[q];
  __syncthreads();
  const int j = threadIdx.x & 31, rl = threadIdx.x >> 5;
  if (j >= ldb) return;
  for (int64_t r = (int64_t)blockIdx.x * 8 + rl; r < n; r += (int64_t)gridDim.x * 8) {
    const double* vr = V + r * pv;
    double s = 0.0;
    for (int i = 0; i < cols; ++i) s = fma(vr[i], sP[i * SV_MAXB + j], s);
    const double w = W[r * ldb + j] - s;
    W[r * ldb + j] = w;
    if (R) R[r * ldb + j] = w;
  }
}

// ------------------------------------------------------------------------------------------------ orth's extra rule
// the first pass of a block's orth: a direction whose norm sqrt(lambda) is not above tau * sigma is dropped as well
__global__ __launch_bounds__(256) void k_svds_trim(const double* __restrict__ dv, double* __restrict__ Minv, int lp, int b, double tau,
                                                   const double* __restrict__ ds) {
  const double floor_abs = tau * ds[0];
  for (int q = threadIdx.x; q < lp * b; q += 256) {
    const int i = q / b, j = q % b;
    if (!(dv[j] > floor_abs)) Minv[i * lp + j] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------------ residuals, flags, info
// part[chunk][i] = the chunk's share of ||R Z[last rows, i]||^2, i < k
__global__ __launch_bounds__(256) void k_svds_resid(const double* __restrict__ R, int ldb, int64_t n, int64_t rpc, const double* __restrict__ Z, int lp,
                                                    const int* __restrict__ st, int k, double* __restrict__ part) {
  __shared__ double sZ[SV_MAXB][SV_MAXM];
  __shared__ double s2[2][SV_MAXM];
  const int cols = st[ST_COLS];
  const int bwl = st[ST_BWL] < cols ? st[ST_BWL] : cols;
  for (int q = threadIdx.x; q < SV_MAXB * SV_MAXM; q += 256) {
    const int j = q / SV_MAXM, c = q % SV_MAXM;
    sZ[j][c] = (j < bwl && c < k) ? Z[(cols - bwl + j) * lp + c] : 0.0;
  }
  __syncthreads();
  const int c = threadIdx.x & (SV_MAXM - 1), rl = threadIdx.x >> 7;
  const int64_t r0 = (int64_t)blockIdx.x * rpc, r1 = r0 + rpc < n ? r0 + rpc : n;
  double acc = 0.0;
  for (int64_t r = r0 + rl; r < r1; r += 2) {
    double y = 0.0;
    for (int j = 0; j < bwl; ++j) y = fma(R[r * ldb + j], sZ[j][c], y);
    acc = fma(y, y, acc);
  }
  s2[rl][c] = acc;
  __syncthreads();
  if (rl == 0) part[(int64_t)blockIdx.x * SV_MAXM + c] = s2[0][c] + s2[1][c];
}

// rho, the flags, residuals = rho / theta, and the info block: cycles, products, n_converged, exhausted, the status word
__global__ __launch_bounds__(SV_MAXM) void k_svds_resid_fin(const double* __restrict__ part, int nch, const double* __restrict__ dv, int k, double tol,
                                                            double tau, const int* __restrict__ st, int cycle, const uint32_t* __restrict__ status,
                                                            double* __restrict__ resid, int64_t* __restrict__ info) {
  const int i = threadIdx.x;
  double s = 0.0;
  for (int ch = 0; ch < nch; ++ch) s += part[(int64_t)ch * SV_MAXM + i];
  const double rho = sqrt(s), th = dv[i < k ? i : 0] * dv[i < k ? i : 0], th1 = dv[0] * dv[0];
  const int conv = (i < k && i < st[ST_COLS] && rho <= fmax(tol * th, tau * th1)) ? 1 : 0;
  const int cnt = __syncthreads_count(conv);
  if (i < k) resid[i] = th > 0.0 ? rho / th : 0.0;
  if (i == 0) {
    info[0] = cycle;
    info[1] = st[ST_PROD];
    info[2] = cnt;
    info[3] = st[ST_EXH];
    info[4] = (int64_t)*status;
  }
}

// ------------------------------------------------------------------------------------------------ restart, rotation
__global__ void k_svds_restart_state(int* __restrict__ st, double* __restrict__ ds, const double* __restrict__ dv, int k, int b) {
  const int cols = st[ST_COLS];
  int nk = k + b < cols - b ? k + b : cols - b;
  const int least = k < cols ? k : cols;
  if (nk < least) nk = least;
  st[ST_ME] = cols;
  st[ST_NK] = nk;
  st[ST_COLS] = nk;
  st[ST_ENDED] = 0;
  st[ST_ACT] = 1;                                             // the projection of R against the kept vectors runs as a step's does
  ds[0] = fmax(ds[0], dv[0] * dv[0]);
}

__global__ __launch_bounds__(256) void k_svds_restart_h(double* __restrict__ H, int lp, const double* __restrict__ dv, const int* __restrict__ st) {
  const int nk = st[ST_NK];
  for (int q = blockIdx.x * 256 + threadIdx.x; q < lp * lp; q += gridDim.x * 256) {
    const int i = q / lp, j = q % lp;
    H[q] = (i == j && i < nk) ? dv[i] * dv[i] : 0.0;
  }
}

// out[:, c] = sum over i < st[me_at] of V[:, i] Z[i][c] for c < nc (nc < 0: st[ST_NK]), zero up to the pitch ldo.  A wave takes
// 4 rows at a time: the rows in LDS, a row of Z per step from L2, lanes on the columns
__global__ __launch_bounds__(256) void k_svds_rotate(const double* __restrict__ V, int64_t n, int pv, const double* __restrict__ Z, int lp,
                                                     const int* __restrict__ st, int me_at, int nc, double* __restrict__ out, int ldo) {
  __shared__ double sRow[4][4][SV_MAXM];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int me = st[me_at];
  if (nc < 0) nc = st[ST_NK];
  for (int64_t r0 = ((int64_t)blockIdx.x * 4 + wv) * 4; r0 < n; r0 += (int64_t)gridDim.x * 16) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const int col = lane + cc * 64;
        sRow[wv][rr][col] = (r0 + rr < n && col < me) ? V[(r0 + rr) * pv + col] : 0.0;
      }
    GFICF_WAVE_SYNC();
    double acc[4][2];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) acc[rr][0] = acc[rr][1] = 0.0;
    for (int i = 0; i < me; ++i) {
      double z[2];
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) z[cc] = lane + cc * 64 < nc ? Z[i * lp + lane + cc * 64] : 0.0;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const double a = sRow[wv][rr][i];
        acc[rr][0] = fma(a, z[0], acc[rr][0]);
        acc[rr][1] = fma(a, z[1], acc[rr][1]);
      }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
      for (int cc = 0; cc < 2; ++cc)
        if (r0 + rr < n && lane + cc * 64 < ldo) out[(r0 + rr) * ldo + lane + cc * 64] = acc[rr][cc];
    GFICF_WAVE_SYNC();
  }
}

// M = (3 I - S) / 2 over the k leading rows and columns, zero elsewhere: Y M is one Newton-Schulz step towards orthonormal
// columns for S = Y'Y close to I; it leaves every column where it is to first order, and a zero column zero
__global__ __launch_bounds__(256) void k_svds_polish(const double* __restrict__ S, int lp, int k, double* __restrict__ M) {
  for (int q = blockIdx.x * 256 + threadIdx.x; q < lp * lp; q += gridDim.x * 256) {
    const int i = q / lp, j = q % lp;
    M[q] = (i < k && j < k) ? (i == j ? 1.5 : 0.0) - 0.5 * S[q] : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------ workspace
struct SvWs {
  uint32_t* status;
  int* st;
  double* ds;
  int64_t* info;
  void* tr_ws;
  size_t tr_bytes;
  int64_t* tptr;
  int32_t* tidx;
  double* tx;
  int64_t *segM, *segT;
  double *part, *mu, *V, *V2, *Q, *Wn, *W2, *Qn, *R, *Tb, *Vk, *Tk, *P, *ppart, *npart, *dvec;
  PcaSmall smB, smH, smK;
};

size_t sv_carve(char* base, int64_t G, int64_t N, int64_t nnz, int k, int b, int m, SvWs& w) {
  gficf_carver cv;
  cv.base = base;
  const size_t n1 = (size_t)(nnz > 0 ? nnz : 1), n = (size_t)(G < N ? G : N), nl = (size_t)(G < N ? N : G);
  const size_t ldb = (size_t)pca_ld(b), ldk = (size_t)pca_ld(k), pv = (size_t)pca_ld(m), nch = (size_t)pca_chunks((int64_t)n);
  w.status = cv.take<uint32_t>(1);
  w.st = cv.take<int>(ST_N);
  w.ds = cv.take<double>(2);
  w.info = cv.take<int64_t>(8);
  w.tr_bytes = gficf_csc_transpose_workspace_bytes(G, N);
  w.tr_ws = cv.take<char>(w.tr_bytes);
  w.tptr = cv.take<int64_t>((size_t)G + 1);
  w.tidx = cv.take<int32_t>(n1);
  w.tx = cv.take<double>(n1);
  w.segM = cv.take<int64_t>((size_t)N + 1);
  w.segT = cv.take<int64_t>((size_t)G + 1);
  w.part = cv.take<double>((size_t)pca_max_units((int64_t)nl, nnz) * (ldb > ldk ? ldb : ldk));
  w.mu = cv.take<double>((size_t)G);
  w.V = cv.take<double>(n * pv);
  w.V2 = cv.take<double>(n * pv);
  w.Q = cv.take<double>(n * ldb);
  w.Wn = cv.take<double>(n * ldb);
  w.W2 = cv.take<double>(n * ldb);
  w.Qn = cv.take<double>(n * ldb);
  w.R = cv.take<double>(n * ldb);
  w.Tb = cv.take<double>(nl * ldb);
  w.Vk = cv.take<double>(n * ldk);                           // (pitch at least 8: they also hold the column of ones behind mu)
  w.Tk = cv.take<double>(nl * ldk);
  w.P = cv.take<double>(SV_PN);
  w.ppart = cv.take<double>(nch * SV_PN);
  w.npart = cv.take<double>((size_t)PCA_CHUNKS * SV_MAXM);
  w.dvec = cv.take<double>(SV_MAXM);
  pca_carve_small(cv, (int64_t)n, b, w.smB);
  pca_carve_small(cv, 1, m, w.smH);
  pca_carve_small(cv, (int64_t)n, k, w.smK);
  return cv.total();
}

int sv_check(int64_t G, int64_t N, int64_t nnz, int k, int b, int m, double tol, int max_cycles) {
  if (G < 1 || N < 1 || nnz < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld, nnz = %lld: the matrix needs a row and a column", (long long)G, (long long)N, (long long)nnz);
  if (G > INT32_MAX || N > INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^31 - 1 genes or cells");
  const int64_t n = G < N ? G : N;
  if (b < 1 || b > SV_MAXB) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "b = %d: the block width must lie in [1, %d]", b, SV_MAXB);
  if (m < b || m > SV_MAXM || m > n) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "m = %d: b = %d <= m <= min(%d, N, G) = %lld is required", m, b, SV_MAXM, (long long)(n < SV_MAXM ? n : SV_MAXM));
  if (k < 1 || k > m || (k + 2 * b > m && m != n))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %d, b = %d, m = %d: 1 <= k and k + 2 b <= m are required (any k <= m when m = min(N, G) = %lld)", k, b, m, (long long)n);
  if (!(tol >= 0.0) || max_cycles < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "tol = %g, max_cycles = %d: tol >= 0 and max_cycles >= 1 are required", tol, max_cycles);
  return GFICF_OK;
}

// ------------------------------------------------------------------------------------------------ the run
struct SvRun {
  gficf_ctx* ctx;
  SvWs w;
  PcaCsc M, T;                  // genes x cells and its transpose
  const double* mu;
  int64_t G, N, n, nl;
  int b, m, k, ldb, ldk, pv, lpB, lpH, lpK;
  bool tr;                      // N < G: the short side is the cells
  double tau;
  int64_t nch, rpc;             // chunks of the n rows of the short side

  // (At X: G rows in, N rows out;  At'X: N rows in, G rows out), l columns
  int to_cells(const double* X, double* out, int l) {
    int r = pca_spmm(ctx, M, X, l, out, w.part, w.status);
    if (!r && mu) r = pca_centre(ctx, X, G, mu, out, N, nullptr, pca_ld(l), w.smB.cpart, w.smB.cvec);
    return r;
  }
  int to_genes(const double* X, double* out, int l) {
    int r = pca_spmm(ctx, T, X, l, out, w.part, w.status);
    if (!r && mu) r = pca_centre(ctx, X, N, nullptr, out, G, mu, pca_ld(l), w.smB.cpart, w.smB.cvec);
    return r;
  }
  int to_big(const double* X, double* out, int l) { return tr ? to_genes(X, out, l) : to_cells(X, out, l); }
  int to_small(const double* X, double* out, int l) { return tr ? to_cells(X, out, l) : to_genes(X, out, l); }

  // s.S = Y'Y for the n x l matrix Y: fixed chunks of rows, added in order
  int gram(const PcaSmall& s, const double* Y, int l) {
    const int ld = pca_ld(l), lp = pca_lp(l);
    const dim3 grid((unsigned)nch), blk(256);
    hipStream_t st = ctx->stream;
    if (lp == 16) hipLaunchKernelGGL(k_pca_gram<1>, grid, blk, 0, st, Y, n, ld, rpc, s.gpart);
    else if (lp == 32) hipLaunchKernelGGL(k_pca_gram<2>, grid, blk, 0, st, Y, n, ld, rpc, s.gpart);
    else if (lp == 64) hipLaunchKernelGGL(k_pca_gram<4>, grid, blk, 0, st, Y, n, ld, rpc, s.gpart);
    else hipLaunchKernelGGL(k_pca_gram<8>, grid, blk, 0, st, Y, n, ld, rpc, s.gpart);
    hipLaunchKernelGGL(k_pca_gram_fin, dim3(pca_grid(lp * lp)), blk, 0, st, (const double*)s.gpart, (int)nch, lp * lp, s.S);
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }

  // P = V'Wn;  Wn -= V P  (R too, if given)
  int project(const double* V) {
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_svds_proj, dim3((unsigned)nch), dim3(256), 0, s, V, pv, (const double*)w.Wn, ldb, n, rpc, (const int*)w.st, w.ppart);
    hipLaunchKernelGGL(k_svds_proj_fin, dim3(SV_PN / 256), dim3(256), 0, s, (const double*)w.ppart, (int)nch, (const int*)w.st, w.P);
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }
  int update(const double* V, double* R) {
    hipLaunchKernelGGL(k_svds_update, dim3(pca_grid(n, 8)), dim3(256), 0, ctx->stream, V, pv, (const double*)w.P, w.Wn, ldb, n, (const int*)w.st, R);
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }

  // Qn = orth(Wn) with the tau * sigma rule; then the new block's width and Q = Qn
  int next_block() {
    hipStream_t s = ctx->stream;
    GFICF_RC(pca_gram_eig(ctx, w.smB, w.Wn, n, b));
    hipLaunchKernelGGL(k_svds_trim, dim3(1), dim3(256), 0, s, (const double*)w.smB.dv, w.smB.Minv, lpB, b, tau, (const double*)w.ds);
    GFICF_RC(pca_apply(ctx, w.Wn, n, b, w.smB.Minv, w.W2));
    GFICF_RC(pca_gram_eig(ctx, w.smB, w.W2, n, b));
    GFICF_RC(pca_apply(ctx, w.W2, n, b, w.smB.Minv, w.Qn));
    return commit(0);
  }
  int commit(int first) {
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_svds_width, dim3(1), dim3(1), 0, s, (const double*)w.smB.dv, b, n, w.st, first);
    hipLaunchKernelGGL(k_svds_copyq, dim3(pca_grid(n * ldb)), dim3(256), 0, s, (const double*)w.Qn, w.Q, n, ldb, (const int*)w.st);
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }

  int step(double* V, int last) {
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_svds_begin, dim3(1), dim3(1), 0, s, w.st, m);
    hipLaunchKernelGGL(k_svds_append, dim3(pca_grid(n * ldb)), dim3(256), 0, s, (const double*)w.Q, ldb, V, pv, n, (const int*)w.st);
    GFICF_HIP_CHECK(hipGetLastError());
    GFICF_RC(to_big(w.Q, w.Tb, b));
    GFICF_RC(to_small(w.Tb, w.Wn, b));
    hipLaunchKernelGGL(k_svds_colss, dim3((unsigned)nch), dim3(256), 0, s, (const double*)w.Wn, n, ldb, rpc, w.npart);
    hipLaunchKernelGGL(k_svds_sigma, dim3(1), dim3(SV_MAXM), 0, s, (const double*)w.npart, (int)nch, b, (const int*)w.st, w.ds);
    GFICF_RC(project(V));
    hipLaunchKernelGGL(k_svds_hfill, dim3(1), dim3(256), 0, s, (const double*)w.P, w.smH.S, lpH, (const int*)w.st);
    GFICF_RC(update(V, nullptr));
    GFICF_RC(project(V));
    GFICF_RC(update(V, w.R));
    hipLaunchKernelGGL(k_svds_step_end, dim3(1), dim3(1), 0, s, w.st, n, b, m, last);
    GFICF_HIP_CHECK(hipGetLastError());
    return next_block();
  }

  // the Ritz step and the read-back: info[0 .. 5)
  int ritz(int cycle, double tol, double* d_resid, int64_t* h_info) {
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_pca_eig, dim3(1), dim3(PCA_EIG_T), 0, s, (const double*)w.smH.S, lpH, m, tau, w.smH.V, w.smH.Minv, w.smH.Mfwd, w.smH.Mkeep, w.smH.dv);
    hipLaunchKernelGGL(k_svds_resid, dim3((unsigned)nch), dim3(256), 0, s, (const double*)w.R, ldb, n, rpc, (const double*)w.smH.Mkeep, lpH, (const int*)w.st, k, w.npart);
    hipLaunchKernelGGL(k_svds_resid_fin, dim3(1), dim3(SV_MAXM), 0, s, (const double*)w.npart, (int)nch, (const double*)w.smH.dv, k, tol, tau, (const int*)w.st,
                       cycle, (const uint32_t*)w.status, d_resid, w.info);
    GFICF_HIP_CHECK(hipGetLastError());
    GFICF_HIP_CHECK(hipMemcpyAsync(h_info, w.info, sizeof(int64_t) * 5, hipMemcpyDeviceToHost, s));
    GFICF_HIP_CHECK(hipStreamSynchronize(s));
    return GFICF_OK;
  }

  // V2 = V Z[:, :nk], H = diag(theta[:nk]), the next block from R
  int restart(const double* V, double* V2) {
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_svds_restart_state, dim3(1), dim3(1), 0, s, w.st, w.ds, (const double*)w.smH.dv, k, b);
    hipLaunchKernelGGL(k_svds_rotate, dim3(pca_grid(n, 16)), dim3(256), 0, s, V, n, pv, (const double*)w.smH.Mkeep, lpH, (const int*)w.st, (int)ST_ME, -1, V2, pv);
    hipLaunchKernelGGL(k_svds_restart_h, dim3(pca_grid(lpH * lpH)), dim3(256), 0, s, w.smH.S, lpH, (const double*)w.smH.dv, (const int*)w.st);
    GFICF_HIP_CHECK(hipGetLastError());
    GFICF_HIP_CHECK(hipMemcpyAsync(w.Wn, w.R, sizeof(double) * (size_t)n * (size_t)ldb, hipMemcpyDeviceToDevice, s));
    GFICF_RC(project(V2));
    GFICF_RC(update(V2, nullptr));
    GFICF_RC(project(V2));
    GFICF_RC(update(V2, nullptr));
    return next_block();
  }
};

}  // namespace

extern "C" {

int gficf_svds_abi_version(void) { return GFICF_SVDS_ABI_VERSION; }

size_t gficf_svds_workspace_bytes(int64_t G, int64_t N, int64_t nnz, int k, int b, int m) {
  if (G < 1 || N < 1 || nnz < 0 || G > INT32_MAX || N > INT32_MAX) return 0;
  const int64_t n = G < N ? G : N;
  if (b < 1 || b > SV_MAXB || m < b || m > SV_MAXM || m > n || k < 1 || k > m || (k + 2 * b > m && m != n)) return 0;
  SvWs w;
  return sv_carve(nullptr, G, N, nnz, k, b, m, w);
}

int gficf_svds_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int64_t nnz,
                      int centre, const double* d_start, int k, int b, int m, double tol, int max_cycles, void* ws, size_t ws_bytes,
                      double* d_d, double* d_cells, double* d_genes, double* d_centre, double* d_residuals, int64_t* d_info) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(sv_check(G, N, nnz, k, b, m, tol, max_cycles));
  if (!d_colptr || !d_start || !ws || !d_d || !d_cells || !d_genes || !d_residuals || !d_info || (centre && !d_centre) || (nnz > 0 && (!d_rowidx || !d_x)))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  SvRun r;
  const size_t need = sv_carve(nullptr, G, N, nnz, k, b, m, r.w);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  sv_carve((char*)ws, G, N, nnz, k, b, m, r.w);
  SvWs& w = r.w;
  r.ctx = ctx;
  r.G = G; r.N = N; r.tr = N < G; r.n = r.tr ? N : G; r.nl = r.tr ? G : N;
  r.b = b; r.m = m; r.k = k;
  r.ldb = pca_ld(b); r.ldk = pca_ld(k); r.pv = pca_ld(m); r.lpB = pca_lp(b); r.lpH = pca_lp(m); r.lpK = pca_lp(k);
  r.tau = pca_tau(G > N ? G : N);
  r.nch = pca_chunks(r.n); r.rpc = gficf_ceil_div(r.n, r.nch);
  r.mu = nullptr;
  const int64_t n = r.n;
  hipStream_t st = ctx->stream;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.st, 0, sizeof(int) * ST_N, st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.ds, 0, sizeof(double) * 2, st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.info, 0, sizeof(int64_t) * 8, st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.smH.S, 0, sizeof(double) * (size_t)r.lpH * (size_t)r.lpH, st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.R, 0, sizeof(double) * (size_t)n * (size_t)r.ldb, st));
  // the gene-major view: M (genes x cells CSC) gives A X = M'X, its transpose T gives A'X = T'X
  GFICF_RC(gficf_csc_transpose_device(ctx, G, N, d_colptr, d_rowidx, d_x, nnz, w.tptr, w.tidx, w.tx, w.tr_ws, w.tr_bytes));
  r.M = PcaCsc{G, N, nnz, d_colptr, d_rowidx, d_x, w.segM, pca_max_units(N, nnz)};
  r.T = PcaCsc{N, G, nnz, w.tptr, w.tidx, w.tx, w.segT, pca_max_units(G, nnz)};
  GFICF_RC(pca_csc_prepare(ctx, r.M, w.status));
  GFICF_RC(pca_csc_prepare(ctx, r.T, w.status));
  if (centre) {                                              // mu = A'1 / N
    double *ones = r.tr ? w.Vk : w.Tk, *sums = r.tr ? w.Tk : w.Vk;
    hipLaunchKernelGGL(k_pca_ones, dim3(pca_grid(N * 8)), dim3(256), 0, st, N, 8, ones);
    GFICF_HIP_CHECK(hipGetLastError());
    GFICF_RC(pca_spmm(ctx, r.T, ones, 1, sums, w.part, w.status));
    hipLaunchKernelGGL(k_pca_copy, dim3(pca_grid(G)), dim3(256), 0, st, G, (const double*)sums, 1.0 / (double)N, (int64_t)8, w.mu);
    hipLaunchKernelGGL(k_pca_copy, dim3(pca_grid(G)), dim3(256), 0, st, G, (const double*)w.mu, 1.0, (int64_t)1, d_centre);
    GFICF_HIP_CHECK(hipGetLastError());
    r.mu = w.mu;
  }
  // Q = orth(start)
  hipLaunchKernelGGL(k_pca_in, dim3(pca_grid(n * r.ldb)), dim3(256), 0, st, n, b, r.ldb, d_start, w.Qn, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  GFICF_RC(pca_orth(ctx, w.smB, w.Qn, w.W2, n, b));
  GFICF_RC(r.commit(1));

  double *V = w.V, *V2 = w.V2;
  int64_t info[5] = {0, 0, 0, 0, 0};
  int nk = 0;
  for (int cycle = 1;; ++cycle) {
    int64_t c = nk;                                          // the cycle's steps at full width
    int steps = 0;
    do {
      c += n - c < b ? n - c : b;
      ++steps;
    } while (c < n && c + (n - c < b ? n - c : b) <= m);
    for (int s = 0; s < steps; ++s) GFICF_RC(r.step(V, s == steps - 1));
    GFICF_RC(r.ritz(cycle, tol, d_residuals, info));
    if (info[4] || info[2] >= k || info[3] || cycle >= max_cycles || m == n) break;
    nk = k + b < (int)c - b ? k + b : (int)c - b;            // (what the device keeps when no block has narrowed; never more)
    GFICF_RC(r.restart(V, V2));
    double* t = V; V = V2; V2 = t;
  }
  // finish: V_k, T = At V_k on the long side, d, the swap back, the sign rule
  const int ldk = r.ldk;
  hipLaunchKernelGGL(k_svds_rotate, dim3(pca_grid(n, 16)), dim3(256), 0, st, (const double*)V, n, r.pv, (const double*)w.smH.Mkeep, r.lpH, (const int*)w.st,
                     (int)ST_COLS, k, w.Tk, ldk);
  GFICF_HIP_CHECK(hipGetLastError());
  // the kept vectors are rotated at every restart and never orthonormalised again: one Newton-Schulz step takes the drift out
  GFICF_RC(r.gram(w.smK, w.Tk, k));
  hipLaunchKernelGGL(k_svds_polish, dim3(pca_grid(r.lpK * r.lpK)), dim3(256), 0, st, (const double*)w.smK.S, r.lpK, k, w.smK.Mkeep);
  GFICF_HIP_CHECK(hipGetLastError());
  GFICF_RC(pca_apply(ctx, w.Tk, n, k, w.smK.Mkeep, w.Vk));
  GFICF_RC(r.to_big(w.Vk, w.Tk, k));
  const int64_t nchl = pca_chunks(r.nl), rpcl = gficf_ceil_div(r.nl, nchl);
  hipLaunchKernelGGL(k_svds_colss, dim3((unsigned)nchl), dim3(256), 0, st, (const double*)w.Tk, r.nl, ldk, rpcl, w.npart);
  hipLaunchKernelGGL(k_svds_dfin, dim3(1), dim3(SV_MAXM), 0, st, (const double*)w.npart, (int)nchl, k, w.dvec);
  if (r.tr) {                                                // genes = T / d, cells = V_k d
    hipLaunchKernelGGL(k_svds_colscale, dim3(pca_grid(r.nl * ldk)), dim3(256), 0, st, w.Tk, r.nl, ldk, k, (const double*)w.dvec, 1);
    hipLaunchKernelGGL(k_svds_colscale, dim3(pca_grid(n * ldk)), dim3(256), 0, st, w.Vk, n, ldk, k, (const double*)w.dvec, 0);
  }
  const double *genes = r.tr ? w.Tk : w.Vk, *cells = r.tr ? w.Vk : w.Tk;
  hipLaunchKernelGGL(k_pca_sign, dim3((unsigned)k), dim3(256), 0, st, genes, G, ldk, w.smB.sgn);
  hipLaunchKernelGGL(k_pca_out, dim3(pca_grid(G * k)), dim3(256), 0, st, G, k, ldk, genes, (const double*)w.smB.sgn, d_genes);
  hipLaunchKernelGGL(k_pca_out, dim3(pca_grid(N * k)), dim3(256), 0, st, N, k, ldk, cells, (const double*)w.smB.sgn, d_cells);
  hipLaunchKernelGGL(k_pca_copy, dim3(1), dim3(256), 0, st, (int64_t)k, (const double*)w.dvec, 1.0, (int64_t)1, d_d);
  GFICF_HIP_CHECK(hipGetLastError());
  GFICF_HIP_CHECK(hipMemcpyAsync(d_info, w.info, sizeof(int64_t) * 4, hipMemcpyDeviceToDevice, st));
  return GFICF_OK;
}

int gficf_svds_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  const int rc = gficf_addon_read_status(ctx, ws, &st);
  if (rc) return rc;
  if (st & PCA_ST_CSC) GFICF_FAIL(GFICF_ERR_BAD_CSC, "a row index out of range or a bad column pointer");
  if (st & PCA_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "a NaN or an infinite value in the matrix or in the start block");
  return GFICF_OK;
}

int gficf_svds_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x,
                    int centre, const double* start, int k, int b, int m, double tol, int max_cycles, double* d, double* cells,
                    double* genes, double* centre_out, double* residuals, int64_t* info) {
  GFICF_CTX_ENTER(ctx);
  if (G < 1 || N < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld: the matrix needs a row and a column", (long long)G, (long long)N);
  if (!colptr || !start || !d || !cells || !genes || !residuals || !info || (centre && !centre_out)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> cp;
  int64_t nnz = 0;
  GFICF_RC(gficf_host_colptr(colptr, colptr_is_i64, N, "colptr", cp, &nnz));
  GFICF_RC(sv_check(G, N, nnz, k, b, m, tol, max_cycles));
  if (nnz > 0 && (!rowidx || !x)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t nsz = (size_t)(nnz > 0 ? nnz : 1), n = (size_t)(G < N ? G : N);
  const size_t wsb = gficf_svds_workspace_bytes(G, N, nnz, k, b, m);
  gficf_host_io io{ctx, "gficf_svds_host"};
  gficf_carver cv;
  int64_t *d_cp, *d_in; int32_t* d_ri; double *d_x, *d_st, *d_dd, *d_ce, *d_ge, *d_mu, *d_rs; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_cp = cv.take<int64_t>((size_t)N + 1); d_ri = cv.take<int32_t>(nsz); d_x = cv.take<double>(nsz);
    d_st = cv.take<double>(n * (size_t)b); d_dd = cv.take<double>((size_t)k); d_ce = cv.take<double>((size_t)N * (size_t)k);
    d_ge = cv.take<double>((size_t)G * (size_t)k); d_mu = cv.take<double>((size_t)G); d_rs = cv.take<double>((size_t)k);
    d_in = cv.take<int64_t>(4);
    d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_cp, cp.data(), sizeof(int64_t) * cp.size());
  io.up(d_ri, rowidx, sizeof(int32_t) * (size_t)nnz);
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  io.up(d_st, start, sizeof(double) * n * (size_t)b);
  int rc = GFICF_OK;
  if (io.ok()) {
    rc = gficf_svds_device(ctx, G, N, d_cp, d_ri, d_x, nnz, centre, d_st, k, b, m, tol, max_cycles, d_ws, wsb, d_dd, d_ce, d_ge, d_mu, d_rs, d_in);
    if (!rc) {
      io.down(d, d_dd, sizeof(double) * (size_t)k);
      io.down(cells, d_ce, sizeof(double) * (size_t)N * (size_t)k);
      io.down(genes, d_ge, sizeof(double) * (size_t)G * (size_t)k);
      io.down(residuals, d_rs, sizeof(double) * (size_t)k);
      io.down(info, d_in, sizeof(int64_t) * 4);
      if (centre) io.down(centre_out, d_mu, sizeof(double) * (size_t)G);
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_svds_sync(ctx, d_ws);
}

}  // extern "C"
