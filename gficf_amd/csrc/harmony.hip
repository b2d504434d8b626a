// harmony.hip — Harmony batch correction of the PCA cells: a soft k-means on the unit sphere with a diversity penalty, then a
// mixture of per-cluster ridge regressions.  Built into libgficf_harmony.so, which links libgficf_hip.so and uses its context and
// error plumbing (include/gficf_harmony.h states the contract, the arithmetic and the order of every sum).
//
// Launches, all on the context's stream (N cells, K clusters, d columns, B levels; a chunk is 1024 cells):
//   normalise   k_hm_normalise                                          one thread a cell
//   start       k_hm_transpose, init_iter x { k_hm_hard, k_hm_centroid_part<hard>, k_hm_centroid_finish }
//   dist        k_hm_transpose (Zc as d x N, read coalesced), k_hm_dist (a thread: one cell, four centroids)
//   assign      k_hm_levels, dist, k_hm_update (no penalty), counts: k_hm_binsum + k_hm_pr, k_hm_binsum, k_hm_oe (set)
//   round       k_hm_levels, k_hm_binsum + k_hm_pr, k_hm_centroid_part<soft>, k_hm_centroid_finish, dist, then a block
//               { k_hm_binsum, k_hm_oe (-), k_hm_update, k_hm_binsum, k_hm_oe (+) }: five launches a block
//   objective   k_hm_levels, dist, k_hm_objective (256 cells a workgroup), k_hm_obj_finish
//   correct     k_hm_levels (pair bins), k_hm_binsum + k_hm_sumparts (Gram entries), k_hm_moment_part + k_hm_sumparts,
//               k_hm_solve (Cholesky, one workgroup a cluster), k_hm_apply
// No floating-point atomics; every grid and block shape is a function of (N, K, d, B, V) alone.
#include <cmath>

#include "addon_status.h"
#include "block_ops.h"
#include "common.h"
#include "gficf_harmony.h"

namespace {

constexpr int HM_CH = 1024;            // cells of a chunk
constexpr uint32_t HM_ST_LEVEL = 1u;   // a level id outside its variable's range
constexpr uint32_t HM_ST_VALUE = 2u;   // a row whose norm is not finite
constexpr uint32_t HM_ST_PERM = 4u;    // an entry of perm outside [0, N)
constexpr int HM_MAX_VX = GFICF_HARMONY_MAX_V + GFICF_HARMONY_MAX_V * (GFICF_HARMONY_MAX_V - 1) / 2;   // variables and pairs of them
constexpr int HM_KB = GFICF_HARMONY_MAX_K * GFICF_HARMONY_MAX_B;
constexpr int HM_NA = GFICF_HARMONY_MAX_B + 1;
constexpr int HM_MOMENT_LDS = 6144;    // doubles of k_hm_moment_part's bins
constexpr size_t HM_MOMENT_CAP = (size_t)256 << 20;   // bytes of the moment partials, before chunks grow

// the bins of the (derived) variables: variable v owns [start[v], start[v + 1]); the first V are the caller's, then the pairs
// (v, v') in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), pair bin = start + (l_v - start_v) * n_v' + (l_v' - start_v')
struct HmBins {
  int V, nv;
  int start[HM_MAX_VX + 1];
};

__global__ __launch_bounds__(256) void k_hm_normalise(int64_t N, int d, const double* Z, double* Zc, uint32_t* st) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const double* z = Z + i * d;
  double s = 0.0;
  for (int j = 0; j < d; ++j) s += z[j] * z[j];
  const double nrm = sqrt(s);
  if (!(nrm < INFINITY)) atomicOr(st, HM_ST_VALUE);
  if (nrm == 0.0) atomicAdd(st + 2, 1u);
  for (int j = 0; j < d; ++j) Zc[i * d + j] = nrm > 0.0 && nrm < INFINITY ? z[j] / nrm : 0.0;
}

// the levels checked; with ext != nullptr also written out, followed by the pair bins (-1 where a level is bad)
__global__ __launch_bounds__(256) void k_hm_levels(int64_t N, HmBins bn, const int32_t* __restrict__ lev, int32_t* __restrict__ ext,
                                                   uint32_t* st) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int32_t l[GFICF_HARMONY_MAX_V];
  bool bad = false;
#pragma unroll
  for (int v = 0; v < GFICF_HARMONY_MAX_V; ++v) {
    l[v] = -1;
    if (v < bn.V) {
      const int32_t x = lev[(int64_t)v * N + i];
      if (x >= bn.start[v] && x < bn.start[v + 1]) l[v] = x; else bad = true;
      if (ext) ext[(int64_t)v * N + i] = l[v];
    }
  }
  if (bad) atomicOr(st, HM_ST_LEVEL);
  if (!ext) return;
  int p = bn.V;
#pragma unroll
  for (int v = 0; v < GFICF_HARMONY_MAX_V; ++v) {
#pragma unroll
    for (int u = v + 1; u < GFICF_HARMONY_MAX_V; ++u) {
      if (u < bn.V) {
        const int nu = bn.start[u + 1] - bn.start[u];
        ext[(int64_t)p * N + i] = l[v] < 0 || l[u] < 0 ? -1 : bn.start[p] + (l[v] - bn.start[v]) * nu + (l[u] - bn.start[u]);
        ++p;
      }
    }
  }
}

// Zt = Zc transposed (d x N): the kernels that walk a cell's columns read it coalesced.  32 cells a workgroup
__global__ __launch_bounds__(256) void k_hm_transpose(int64_t N, int d, const double* __restrict__ Zc, double* __restrict__ Zt) {
  __shared__ double tile[32 * GFICF_HARMONY_MAX_D];
  const int64_t i0 = (int64_t)blockIdx.x * 32;
  const int cnt = N - i0 < 32 ? (int)(N - i0) : 32;
  for (int e = threadIdx.x; e < cnt * d; e += 256) tile[e] = Zc[i0 * d + e];
  __syncthreads();
  for (int e = threadIdx.x; e < 32 * d; e += 256) {
    const int j = e >> 5, c = e & 31;
    if (c < cnt) Zt[(int64_t)j * N + i0 + c] = tile[c * d + j];
  }
}

// dist[k, i] = 2 (1 - Y[k] . Zc[i]), the columns in order; grid (cells / 256, ceil(K / 4)): a thread takes four centroids
__global__ __launch_bounds__(256) void k_hm_dist(int64_t N, int d, int K, const double* __restrict__ Zt, const double* __restrict__ Y,
                                                 double* __restrict__ dist) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int k0 = blockIdx.y * 4;
  if (i >= N) return;
  const double* y[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) y[q] = Y + (int64_t)(k0 + q < K ? k0 + q : K - 1) * d;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < d; ++j) {
    const double z = Zt[(int64_t)j * N + i];
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += y[q][j] * z;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (k0 + q < K) dist[(int64_t)(k0 + q) * N + i] = 2.0 * (1.0 - s[q]);
}

// the centroid of largest dot product, the lowest k on a tie
__global__ __launch_bounds__(256) void k_hm_hard(int64_t N, int d, int K, const double* __restrict__ Zt, const double* __restrict__ Y,
                                                 int32_t* __restrict__ lab) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double best = -INFINITY;
  int32_t at = 0;
  for (int k = 0; k < K; ++k) {
    const double* y = Y + (int64_t)k * d;
    double s = 0.0;
    for (int j = 0; j < d; ++j) s += y[j] * Zt[(int64_t)j * N + i];
    if (s > best) { best = s; at = k; }
  }
  lab[i] = at;
}

// part[c][k][j] = sum over the cells i of chunk c of w[k, i] X[i, j], w = R or (lab == k); grid (chunks, ceil(K / 4)), block = the
// columns (64 or 128): thread j walks the chunk's cells in order
template <bool HARD>
__global__ __launch_bounds__(128) void k_hm_centroid_part(int64_t N, int d, int K, const double* __restrict__ X, const double* __restrict__ R,
                                                          const int32_t* __restrict__ lab, double* __restrict__ part) {
  const int j = threadIdx.x;
  const int64_t c = blockIdx.x;
  const int k0 = blockIdx.y * 4;
  if (j >= d) return;
  const int64_t i0 = c * HM_CH, i1 = i0 + HM_CH < N ? i0 + HM_CH : N;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = i0; i < i1; ++i) {
    const double z = X[i * d + j];
    if (HARD) {
      const int32_t l = lab[i];
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] += l == k0 + q ? z : 0.0;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] += (k0 + q < K ? R[(int64_t)(k0 + q) * N + i] : 0.0) * z;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (k0 + q < K) part[(c * K + (k0 + q)) * d + j] = a[q];
}

// Y[k] = s / |s|, s the chunk sums added in order; a sum of norm 0 leaves Y[k] as it is.  grid K, block 128
__global__ __launch_bounds__(128) void k_hm_centroid_finish(int64_t nch, int d, int K, const double* __restrict__ part, double* __restrict__ Y) {
  __shared__ double sm[GFICF_HARMONY_MAX_D];
  __shared__ double nrm_s;
  const int j = threadIdx.x, k = blockIdx.x;
  double s = 0.0;
  if (j < d)
    for (int64_t c = 0; c < nch; ++c) s += part[(c * K + k) * d + j];
  sm[j] = s;
  __syncthreads();
  if (j == 0) {
    double n2 = 0.0;
    for (int q = 0; q < d; ++q) n2 += sm[q] * sm[q];
    nrm_s = sqrt(n2);
  }
  __syncthreads();
  const double nrm = nrm_s;
  if (j < d && nrm > 0.0 && nrm < INFINITY) Y[(int64_t)k * d + j] = s / nrm;
}

// part[c][k][bin] = sum over the cells at list positions [1024 c, 1024 c + 1024) of w[k, i] [cell i is in bin]; w = R or 1.
// grid (chunks of the list, K or 1); dynamic LDS: 1024 f64 and nv x 1024 int32
__global__ __launch_bounds__(256) void k_hm_binsum(int64_t N, int64_t n, const int32_t* __restrict__ list, const double* __restrict__ R,
                                                   const int32_t* __restrict__ lev, HmBins bn, double* __restrict__ part, uint32_t* st) {
  extern __shared__ double hm_dyn[];
  double* r = hm_dyn;
  int32_t* lv = (int32_t*)(hm_dyn + HM_CH);
  const int t = threadIdx.x, k = blockIdx.y;
  const int64_t c = blockIdx.x, p0 = c * HM_CH;
  for (int p = t; p < HM_CH; p += 256) {
    int64_t i = -1;
    if (p0 + p < n) {
      i = list ? (int64_t)list[p0 + p] : p0 + p;
      if (i < 0 || i >= N) { atomicOr(st, HM_ST_PERM); i = -1; }
    }
    r[p] = i < 0 ? 0.0 : R ? R[(int64_t)k * N + i] : 1.0;
    for (int v = 0; v < bn.nv; ++v) {
      int32_t l = i < 0 ? -1 : lev[(int64_t)v * N + i];
      if (l < bn.start[v] || l >= bn.start[v + 1]) l = -1;
      lv[v * HM_CH + p] = l;
    }
  }
  __syncthreads();
  const int nb = bn.start[bn.nv];
  for (int e = t; e < nb * 4; e += 256) {                     // the four lanes of a quad: the four quarters of one bin
    const int bin = e >> 2, sub = e & 3;
    int v = 0;
    while (bin >= bn.start[v + 1]) ++v;
    const int32_t* l = lv + v * HM_CH + sub * 256;
    const double* rr = r + sub * 256;
    double a = 0.0;
    for (int q = 0; q < 256; ++q) {
      const int qq = (q + sub) & 255;                           // rotated: the quarters meet different LDS banks
      a += l[qq] == bin ? rr[qq] : 0.0;
    }
    a += __shfl_xor(a, 1);
    a += __shfl_xor(a, 2);
    if (sub == 0) part[(c * gridDim.y + k) * nb + bin] = a;
  }
}

// out[e] = the chunk sums of entry e added in order, e < n_out
__global__ __launch_bounds__(256) void k_hm_sumparts(int64_t nch, int64_t n_out, const double* __restrict__ part, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_out) return;
  double s = 0.0;
  for (int64_t c = 0; c < nch; ++c) s += part[c * n_out + e];
  out[e] = s;
}

__global__ __launch_bounds__(64) void k_hm_pr(int64_t nch, int B, int64_t N, const double* __restrict__ part, double* __restrict__ pr) {
  const int b = threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int64_t c = 0; c < nch; ++c) s += part[c * B + b];
  pr[b] = s / (double)N;
}

// the chunk sums of a list folded into O and E: mode 0 sets them, +1 / -1 adds / subtracts.  grid K, block 64
__global__ __launch_bounds__(64) void k_hm_oe(int64_t nch, int K, int B, int n0, const double* __restrict__ part, const double* __restrict__ pr,
                                              int mode, double* __restrict__ O, double* __restrict__ E) {
  __shared__ double sm[GFICF_HARMONY_MAX_B];
  const int b = threadIdx.x, k = blockIdx.x;
  double s = 0.0;
  if (b < B)
    for (int64_t c = 0; c < nch; ++c) s += part[(c * K + k) * B + b];
  sm[b] = s;
  __syncthreads();
  if (b >= B) return;
  double S = 0.0;
  for (int q = 0; q < n0; ++q) S += sm[q];
  const double e = S * pr[b];
  const int64_t at = (int64_t)k * B + b;
  if (mode == 0) { O[at] = s; E[at] = e; }
  else if (mode > 0) { O[at] = O[at] + s; E[at] = E[at] + e; }
  else { O[at] = O[at] - s; E[at] = E[at] - e; }
}

// R of the cells of a list from dist, with the diversity penalty where theta is given
__global__ __launch_bounds__(256) void k_hm_update(int64_t N, int64_t n, const int32_t* __restrict__ list, int K, int V, int B,
                                                   const int32_t* __restrict__ lev, const double* __restrict__ dist, const double* __restrict__ O,
                                                   const double* __restrict__ E, const double* __restrict__ theta, double sigma,
                                                   double* __restrict__ R, uint32_t* st) {
  __shared__ double F[HM_KB];
  const bool pen = theta != nullptr;
  if (pen)
    for (int e = threadIdx.x; e < K * B; e += 256) F[e] = pow((E[e] + 1.0) / (O[e] + 1.0), theta[e % B]);
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int64_t i = list ? (int64_t)list[p] : p;
  if (i < 0 || i >= N) { atomicOr(st, HM_ST_PERM); return; }
  int32_t b[GFICF_HARMONY_MAX_V];
#pragma unroll
  for (int v = 0; v < GFICF_HARMONY_MAX_V; ++v) {
    b[v] = -1;
    if (pen && v < V) {
      const int32_t l = lev[(int64_t)v * N + i];
      b[v] = l >= 0 && l < B ? l : -1;
    }
  }
  double mn = INFINITY;
  for (int k = 0; k < K; ++k) mn = fmin(mn, dist[(int64_t)k * N + i]);
  double s = 0.0;
  for (int k = 0; k < K; ++k) {
    double e = exp(-(dist[(int64_t)k * N + i] - mn) / sigma);
#pragma unroll
    for (int v = 0; v < GFICF_HARMONY_MAX_V; ++v)
      if (b[v] >= 0) e = e * F[k * B + b[v]];
    R[(int64_t)k * N + i] = e;
    s += e;
  }
  for (int k = 0; k < K; ++k) R[(int64_t)k * N + i] = R[(int64_t)k * N + i] / s;
}

// the objective of 256 cells a workgroup
__global__ __launch_bounds__(256) void k_hm_objective(int64_t N, int K, int V, int B, const int32_t* __restrict__ lev, const double* __restrict__ dist,
                                                      const double* __restrict__ R, const double* __restrict__ O, const double* __restrict__ E,
                                                      const double* __restrict__ theta, double sigma, double* __restrict__ part) {
  __shared__ double L[HM_KB];
  __shared__ double red[256];
  for (int e = threadIdx.x; e < K * B; e += 256) L[e] = theta[e % B] * log((O[e] + 1.0) / (E[e] + 1.0));
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double acc = 0.0;
  if (i < N) {
    int32_t b[GFICF_HARMONY_MAX_V];
#pragma unroll
    for (int v = 0; v < GFICF_HARMONY_MAX_V; ++v) {
      b[v] = -1;
      if (v < V) {
        const int32_t l = lev[(int64_t)v * N + i];
        b[v] = l >= 0 && l < B ? l : -1;
      }
    }
    for (int k = 0; k < K; ++k) {
      const double r = R[(int64_t)k * N + i];
      double pe = 0.0;
#pragma unroll
      for (int v = 0; v < GFICF_HARMONY_MAX_V; ++v)
        if (b[v] >= 0) pe += L[k * B + b[v]];
      const double ent = r > 0.0 ? r * log(r) : 0.0;
      acc += r * dist[(int64_t)k * N + i] + sigma * ent + sigma * (r * pe);
    }
  }
  const double s = gficf_block_sum_f64(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_hm_obj_finish(int64_t n, const double* __restrict__ part, double* __restrict__ obj) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int64_t q = threadIdx.x; q < n; q += 256) acc += part[q];
  const double s = gficf_block_sum_f64(acc, red);
  if (threadIdx.x == 0) obj[0] = s;
}

// part[c][k][b][j] = sum over the cells i of chunk c (chm cells) in level b of R[k, i] Z[i, j]; grid (chunks, K, level tiles of
// bt), block = the columns (64 or 128); thread j owns column j of the LDS bins
__global__ __launch_bounds__(128) void k_hm_moment_part(int64_t N, int d, int K, int V, int B, int64_t chm, int bt, const double* __restrict__ Z,
                                                        const double* __restrict__ R, const int32_t* __restrict__ lev, double* __restrict__ part) {
  __shared__ double acc[HM_MOMENT_LDS];
  const int j = threadIdx.x, LJ = blockDim.x, k = blockIdx.y, b0 = blockIdx.z * bt;
  const int64_t c = blockIdx.x;
  const int nbt = B - b0 < bt ? B - b0 : bt;
  for (int b = 0; b < nbt; ++b) acc[b * LJ + j] = 0.0;
  const int64_t i0 = c * chm, i1 = i0 + chm < N ? i0 + chm : N;
  if (j < d) {
    for (int64_t i = i0; i < i1; ++i) {
      const double rz = R[(int64_t)k * N + i] * Z[i * d + j];
      for (int v = 0; v < V; ++v) {
        const int b = lev[(int64_t)v * N + i] - b0;
        if (b >= 0 && b < nbt) acc[b * LJ + j] += rz;
      }
    }
    for (int b = 0; b < nbt; ++b) part[((c * K + k) * B + (b0 + b)) * d + j] = acc[b * LJ + j];
  }
}

// W_k = A_k^-1 (Phi* R_k Z), W_k[0] = 0; grid K, block 256.  Q: K x nbx bin sums of R (levels, then pair bins), M: K x B x d
__global__ __launch_bounds__(256) void k_hm_solve(int d, int B, HmBins bn, const double* __restrict__ Q, const double* __restrict__ M,
                                                  const double* __restrict__ lambda, double* __restrict__ W, uint32_t* st) {
  __shared__ double A[HM_NA * HM_NA];
  __shared__ int bad_s;
  const int t = threadIdx.x, k = blockIdx.x, n = B + 1, nbx = bn.start[bn.nv];
  const double* q = Q + (int64_t)k * nbx;
  double* w = W + (int64_t)k * n * d;
  for (int e = t; e < n * n; e += 256) A[e] = 0.0;
  if (t == 0) bad_s = 0;
  __syncthreads();
  if (t == 0) {
    double S = 0.0;
    for (int b = 0; b < bn.start[1]; ++b) S += q[b];
    A[0] = S;
  }
  for (int b = t; b < B; b += 256) {
    A[(1 + b) * n] = q[b];
    A[1 + b] = q[b];
    A[(1 + b) * n + 1 + b] = q[b] + lambda[b];
  }
  {
    int p = bn.V;
    for (int v = 0; v < bn.V; ++v)
      for (int u = v + 1; u < bn.V; ++u, ++p) {
        const int nu = bn.start[u + 1] - bn.start[u], cnt = bn.start[p + 1] - bn.start[p];
        for (int e = t; e < cnt; e += 256) {
          const int bv = bn.start[v] + e / nu, bu = bn.start[u] + e % nu;
          const double x = q[bn.start[p] + e];
          A[(1 + bv) * n + 1 + bu] = x;
          A[(1 + bu) * n + 1 + bv] = x;
        }
      }
  }
  // the right-hand sides: row 0 is the sum of variable 0's rows
  const double* m = M + (int64_t)k * B * d;
  for (int e = t; e < B * d; e += 256) w[d + e] = m[e];
  for (int j = t; j < d; j += 256) {
    double s = 0.0;
    for (int b = 0; b < bn.start[1]; ++b) s += m[b * d + j];
    w[j] = s;
  }
  __syncthreads();
  // Cholesky, lower triangle in place
  for (int p = 0; p < n; ++p) {
    const double piv = A[p * n + p];
    __syncthreads();
    if (!(piv > 0.0) || !(piv < INFINITY)) {
      if (t == 0) bad_s = 1;
      break;                                                   // piv is the same in every thread
    }
    const double sq = sqrt(piv);
    if (t == 0) A[p * n + p] = sq;
    for (int r = p + 1 + t; r < n; r += 256) A[r * n + p] = A[r * n + p] / sq;
    __syncthreads();
    const int m1 = n - p - 1;
    for (int e = t; e < m1 * m1; e += 256) {
      const int r = p + 1 + e / m1, c = p + 1 + e % m1;
      if (c <= r) A[r * n + c] -= A[r * n + p] * A[c * n + p];
    }
    __syncthreads();
  }
  __syncthreads();
  if (bad_s) {
    for (int e = t; e < n * d; e += 256) w[e] = 0.0;
    if (t == 0) atomicAdd(st + 1, 1u);
    return;
  }
  __threadfence_block();
  for (int j = t; j < d; j += 256) {                           // column j of the right-hand side is this thread's own
    for (int a = 0; a < n; ++a) {
      double s = w[a * d + j];
      for (int c = 0; c < a; ++c) s -= A[a * n + c] * w[c * d + j];
      w[a * d + j] = s / A[a * n + a];
    }
    for (int a = n - 1; a >= 0; --a) {
      double s = w[a * d + j];
      for (int c = a + 1; c < n; ++c) s -= A[c * n + a] * w[c * d + j];
      w[a * d + j] = s / A[a * n + a];
    }
    w[j] = 0.0;
  }
}

// Zcorr[i] = Z[i] - sum_k R[k, i] sum_v W_k[1 + b_v]; block 256 = (256 / LJ) cells x LJ columns
__global__ __launch_bounds__(256) void k_hm_apply(int64_t N, int d, int K, int V, int B, int LJ, const double* __restrict__ Z,
                                                  const int32_t* __restrict__ lev, const double* __restrict__ R, const double* __restrict__ W,
                                                  double* __restrict__ Zcorr) {
  const int j = threadIdx.x % LJ;
  const int64_t i = (int64_t)blockIdx.x * (256 / LJ) + threadIdx.x / LJ;
  if (i >= N || j >= d) return;
  int32_t b[GFICF_HARMONY_MAX_V];
#pragma unroll
  for (int v = 0; v < GFICF_HARMONY_MAX_V; ++v) {
    b[v] = -1;
    if (v < V) {
      const int32_t l = lev[(int64_t)v * N + i];
      b[v] = l >= 0 && l < B ? l : -1;
    }
  }
  double s = 0.0;
  for (int k = 0; k < K; ++k) {
    const double* w = W + (int64_t)k * (B + 1) * d;
    double x = 0.0;
#pragma unroll
    for (int v = 0; v < GFICF_HARMONY_MAX_V; ++v)
      if (b[v] >= 0) x += w[(1 + b[v]) * d + j];
    s += R[(int64_t)k * N + i] * x;
  }
  Zcorr[i * d + j] = Z[i * d + j] - s;
}

// ---------------------------------------------------------------- host side

struct HmShape {
  int64_t N;
  int d, K, V, B, LJ;
  int64_t nch;        // chunks of 1024 cells
  int64_t chm, nchm;  // the moments' chunk and their number
  int bt;             // levels a workgroup of k_hm_moment_part bins
  int64_t pmax;       // most pair bins V variables of B levels can have
};

struct HmWs {
  uint32_t* status;   // [0] status bits, [1] clusters left out, [2] zero rows
  double *dist, *zt, *cpart, *bpart, *mpart, *Q, *M, *W, *pr, *opart, *obj;
  int32_t *ext, *lab;
};

static int hm_shape(int64_t N, int64_t d, int64_t K, int64_t V, int64_t B, HmShape& s) {
  if (d > GFICF_HARMONY_MAX_D || K > GFICF_HARMONY_MAX_K || B > GFICF_HARMONY_MAX_B || V > GFICF_HARMONY_MAX_V || N > INT32_MAX)
    GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "N = %lld, d = %lld, K = %lld, V = %lld, B = %lld: at most 2^31 - 1, %d, %d, %d, %d", (long long)N, (long long)d,
               (long long)K, (long long)V, (long long)B, GFICF_HARMONY_MAX_D, GFICF_HARMONY_MAX_K, GFICF_HARMONY_MAX_V, GFICF_HARMONY_MAX_B);
  if (N < 1 || d < 1 || K < 1 || V < 1 || B < V || K > N)
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld, d = %lld, K = %lld, V = %lld, B = %lld: a size is out of range", (long long)N, (long long)d,
               (long long)K, (long long)V, (long long)B);
  s.N = N; s.d = (int)d; s.K = (int)K; s.V = (int)V; s.B = (int)B;
  s.LJ = d <= 64 ? 64 : 128;
  s.nch = gficf_ceil_div(N, HM_CH);
  s.chm = HM_CH;
  while ((size_t)gficf_ceil_div(N, s.chm) * (size_t)(K * B * d) * sizeof(double) > HM_MOMENT_CAP) s.chm *= 2;
  s.nchm = gficf_ceil_div(N, s.chm);
  s.bt = HM_MOMENT_LDS / s.LJ;
  s.pmax = V > 1 ? (B * B * (V - 1)) / (2 * V) + 1 : 0;
  return GFICF_OK;
}

static size_t hm_carve(char* base, const HmShape& s, HmWs& w) {
  gficf_carver cv;
  cv.base = base;
  const size_t N = (size_t)s.N, K = (size_t)s.K, B = (size_t)s.B, d = (size_t)s.d, nbx = B + (size_t)s.pmax;
  w.status = cv.take<uint32_t>(4);
  w.obj = cv.take<double>(1);
  w.pr = cv.take<double>(B);
  w.dist = cv.take<double>(K * N);
  w.zt = cv.take<double>(N * d);
  w.cpart = cv.take<double>((size_t)s.nch * K * d);
  w.bpart = cv.take<double>((size_t)s.nch * K * nbx);
  w.mpart = cv.take<double>((size_t)s.nchm * K * B * d);
  w.Q = cv.take<double>(K * nbx);
  w.M = cv.take<double>(K * B * d);
  w.W = cv.take<double>(K * (B + 1) * d);
  w.opart = cv.take<double>((size_t)gficf_ceil_div(s.N, 256));
  w.ext = cv.take<int32_t>((size_t)HM_MAX_VX * N);
  w.lab = cv.take<int32_t>(N);
  return cv.total();
}

static int hm_bins(const HmShape& s, const int32_t* var_start, HmBins& bn) {
  if (!var_start) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL var_start");
  if (var_start[0] != 0 || var_start[s.V] != s.B) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "var_start must run from 0 to B = %d", s.B);
  for (int v = 0; v < s.V; ++v)
    if (var_start[v + 1] <= var_start[v]) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "variable %d has no level", v);
  bn.V = s.V;
  for (int v = 0; v <= s.V; ++v) bn.start[v] = var_start[v];
  int p = s.V;
  for (int v = 0; v < s.V; ++v)
    for (int u = v + 1; u < s.V; ++u, ++p)
      bn.start[p + 1] = bn.start[p] + (var_start[v + 1] - var_start[v]) * (var_start[u + 1] - var_start[u]);
  bn.nv = p;
  for (int v = p + 1; v <= HM_MAX_VX; ++v) bn.start[v] = bn.start[p];
  return GFICF_OK;
}

// what every entry does first
struct HmRun {
  gficf_ctx* ctx;
  hipStream_t st;
  HmShape s;
  HmWs w;
  HmBins bn;      // the caller's variables only (nv = V)
  HmBins bx;      // with the pair bins
};

static int hm_enter(HmRun& r, gficf_ctx* ctx, int64_t N, int64_t d, int64_t K, int64_t V, int64_t B, const int32_t* var_start, void* ws,
                    size_t ws_bytes) {
  r.ctx = ctx;
  r.st = ctx->stream;
  GFICF_RC(hm_shape(N, d, K, V, B, r.s));
  if (var_start) {
    GFICF_RC(hm_bins(r.s, var_start, r.bx));
    r.bn = r.bx;
    r.bn.nv = r.s.V;
  }
  if (!ws) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL workspace");
  return gficf_addon_carve(ws, ws_bytes, [&](char* base) { return hm_carve(base, r.s, r.w); });
}

static unsigned hm_cells(int64_t n) { return (unsigned)gficf_ceil_div(n > 0 ? n : 1, 256); }

static void hm_binsum(HmRun& r, int64_t n, const int32_t* list, const double* R, const int32_t* lev, const HmBins& bn, double* part) {
  const size_t lds = HM_CH * sizeof(double) + (size_t)bn.nv * HM_CH * sizeof(int32_t);
  hipLaunchKernelGGL(k_hm_binsum, dim3((unsigned)gficf_ceil_div(n, HM_CH), R ? r.s.K : 1), dim3(256), lds, r.st, r.s.N, n, list, R, lev, bn, part,
                     r.w.status);
}

static void hm_levels_pr(HmRun& r, const int32_t* lev) {
  hipLaunchKernelGGL(k_hm_levels, dim3(hm_cells(r.s.N)), dim3(256), 0, r.st, r.s.N, r.bn, lev, (int32_t*)nullptr, r.w.status);
  hm_binsum(r, r.s.N, nullptr, nullptr, lev, r.bn, r.w.bpart);
  hipLaunchKernelGGL(k_hm_pr, dim3(1), dim3(64), 0, r.st, r.s.nch, r.s.B, r.s.N, r.w.bpart, r.w.pr);
}

static void hm_transpose(HmRun& r, const double* Zc) {
  hipLaunchKernelGGL(k_hm_transpose, dim3((unsigned)gficf_ceil_div(r.s.N, 32)), dim3(256), 0, r.st, r.s.N, r.s.d, Zc, r.w.zt);
}

static void hm_dist(HmRun& r, const double* Zc, const double* Y) {
  hm_transpose(r, Zc);
  hipLaunchKernelGGL(k_hm_dist, dim3(hm_cells(r.s.N), (unsigned)gficf_ceil_div(r.s.K, 4)), dim3(256), 0, r.st, r.s.N, r.s.d, r.s.K, r.w.zt, Y, r.w.dist);
}

template <bool HARD>
static void hm_centroids(HmRun& r, const double* Zc, const double* R, const int32_t* lab, double* Y) {
  hipLaunchKernelGGL(k_hm_centroid_part<HARD>, dim3((unsigned)r.s.nch, (unsigned)gficf_ceil_div(r.s.K, 4)), dim3(r.s.LJ), 0, r.st, r.s.N, r.s.d,
                     r.s.K, Zc, R, lab, r.w.cpart);
  hipLaunchKernelGGL(k_hm_centroid_finish, dim3(r.s.K), dim3(128), 0, r.st, r.s.nch, r.s.d, r.s.K, r.w.cpart, Y);
}

static void hm_update(HmRun& r, int64_t n, const int32_t* list, const int32_t* lev, const double* O, const double* E, const double* theta,
                      double sigma, double* R) {
  hipLaunchKernelGGL(k_hm_update, dim3(hm_cells(n)), dim3(256), 0, r.st, r.s.N, n, list, r.s.K, r.s.V, r.s.B, lev, r.w.dist, O, E, theta, sigma, R,
                     r.w.status);
}

static void hm_oe(HmRun& r, int64_t n, int mode, double* O, double* E) {
  hipLaunchKernelGGL(k_hm_oe, dim3(r.s.K), dim3(64), 0, r.st, gficf_ceil_div(n, HM_CH), r.s.K, r.s.B, r.bn.start[1], r.w.bpart, r.w.pr, mode, O, E);
}

static int hm_sigma(double sigma) {
  if (!(sigma > 0.0) || !(sigma < INFINITY)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "sigma = %g: it must be positive and finite", sigma);
  return GFICF_OK;
}

}  // namespace

extern "C" {

int gficf_harmony_abi_version(void) { return GFICF_HARMONY_ABI_VERSION; }

size_t gficf_harmony_workspace_bytes(int64_t N, int64_t d, int64_t K, int64_t V, int64_t B) {
  if (d > GFICF_HARMONY_MAX_D || K > GFICF_HARMONY_MAX_K || B > GFICF_HARMONY_MAX_B || V > GFICF_HARMONY_MAX_V || N > INT32_MAX || N < 1 || d < 1 ||
      K < 1 || V < 1 || B < V || K > N)
    return 0;
  HmShape s;
  HmWs w;
  if (hm_shape(N, d, K, V, B, s)) return 0;
  return hm_carve(nullptr, s, w);
}

int gficf_harmony_normalise_device(gficf_ctx* ctx, int64_t N, int64_t d, const double* d_Z, double* d_Zc, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  if (d > GFICF_HARMONY_MAX_D || N > INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "N = %lld, d = %lld: at most 2^31 - 1, %d", (long long)N, (long long)d,
                                                           GFICF_HARMONY_MAX_D);
  if (N < 1 || d < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld, d = %lld: a size is out of range", (long long)N, (long long)d);
  if (!d_Z || !d_Zc || !ws) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (ws_bytes < 16) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "workspace too small");
  GFICF_HIP_CHECK(hipMemsetAsync(ws, 0, 16, ctx->stream));
  hipLaunchKernelGGL(k_hm_normalise, dim3(hm_cells(N)), dim3(256), 0, ctx->stream, N, (int)d, d_Z, d_Zc, (uint32_t*)ws);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_harmony_start_device(gficf_ctx* ctx, int64_t N, int64_t d, int64_t K, const double* d_Zc, const double* d_Y0, int32_t init_iter,
                               double* d_Y, int32_t* d_labels, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  HmRun r;
  GFICF_RC(hm_enter(r, ctx, N, d, K, 1, 1, nullptr, ws, ws_bytes));
  if (init_iter < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "init_iter = %d", (int)init_iter);
  if (!d_Zc || !d_Y0 || !d_Y || !d_labels) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (d_Y != d_Y0) GFICF_HIP_CHECK(hipMemcpyAsync(d_Y, d_Y0, sizeof(double) * (size_t)(K * d), hipMemcpyDeviceToDevice, r.st));
  GFICF_HIP_CHECK(hipMemsetAsync(d_labels, 0, sizeof(int32_t) * (size_t)N, r.st));
  if (init_iter > 0) hm_transpose(r, d_Zc);
  for (int it = 0; it < init_iter; ++it) {
    hipLaunchKernelGGL(k_hm_hard, dim3(hm_cells(N)), dim3(256), 0, r.st, N, r.s.d, r.s.K, r.w.zt, d_Y, d_labels);
    hm_centroids<true>(r, d_Zc, nullptr, d_labels, d_Y);
  }
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_harmony_assign_device(gficf_ctx* ctx, int64_t N, int64_t d, int64_t K, int64_t V, int64_t B, const int32_t* var_start,
                                const double* d_Zc, const int32_t* d_levels, const double* d_Y, double sigma, double* d_R, double* d_O,
                                double* d_E, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  HmRun r;
  if (!var_start) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL var_start");
  GFICF_RC(hm_enter(r, ctx, N, d, K, V, B, var_start, ws, ws_bytes));
  GFICF_RC(hm_sigma(sigma));
  if (!d_Zc || !d_levels || !d_Y || !d_R || !d_O || !d_E) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  hm_levels_pr(r, d_levels);
  hm_dist(r, d_Zc, d_Y);
  hm_update(r, N, nullptr, d_levels, d_O, d_E, nullptr, sigma, d_R);
  hm_binsum(r, N, nullptr, d_R, d_levels, r.bn, r.w.bpart);
  hm_oe(r, N, 0, d_O, d_E);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_harmony_round_device(gficf_ctx* ctx, int64_t N, int64_t d, int64_t K, int64_t V, int64_t B, const int32_t* var_start,
                               const double* d_Zc, const int32_t* d_levels, const double* d_theta, double sigma, const int32_t* d_perm,
                               int32_t n_blocks, double* d_R, double* d_O, double* d_E, double* d_Y, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  HmRun r;
  if (!var_start) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL var_start");
  GFICF_RC(hm_enter(r, ctx, N, d, K, V, B, var_start, ws, ws_bytes));
  GFICF_RC(hm_sigma(sigma));
  if (n_blocks < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_blocks = %d", (int)n_blocks);
  if (!d_Zc || !d_levels || !d_theta || !d_perm || !d_R || !d_O || !d_E || !d_Y) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  hm_levels_pr(r, d_levels);
  hm_centroids<false>(r, d_Zc, d_R, nullptr, d_Y);
  hm_dist(r, d_Zc, d_Y);
  const int64_t q = N / n_blocks, rem = N % n_blocks;
  int64_t off = 0;
  for (int64_t t = 0; t < n_blocks; ++t) {
    const int64_t len = q + (t < rem ? 1 : 0);
    if (len == 0) continue;
    const int32_t* list = d_perm + off;
    hm_binsum(r, len, list, d_R, d_levels, r.bn, r.w.bpart);
    hm_oe(r, len, -1, d_O, d_E);
    hm_update(r, len, list, d_levels, d_O, d_E, d_theta, sigma, d_R);
    hm_binsum(r, len, list, d_R, d_levels, r.bn, r.w.bpart);
    hm_oe(r, len, +1, d_O, d_E);
    off += len;
  }
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_harmony_objective_device(gficf_ctx* ctx, int64_t N, int64_t d, int64_t K, int64_t V, int64_t B, const int32_t* var_start,
                                   const double* d_Zc, const int32_t* d_levels, const double* d_Y, const double* d_R, const double* d_O,
                                   const double* d_E, const double* d_theta, double sigma, double* d_obj, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  HmRun r;
  if (!var_start) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL var_start");
  GFICF_RC(hm_enter(r, ctx, N, d, K, V, B, var_start, ws, ws_bytes));
  GFICF_RC(hm_sigma(sigma));
  if (!d_Zc || !d_levels || !d_Y || !d_R || !d_O || !d_E || !d_theta || !d_obj) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  hipLaunchKernelGGL(k_hm_levels, dim3(hm_cells(N)), dim3(256), 0, r.st, N, r.bn, d_levels, (int32_t*)nullptr, r.w.status);
  hm_dist(r, d_Zc, d_Y);
  hipLaunchKernelGGL(k_hm_objective, dim3(hm_cells(N)), dim3(256), 0, r.st, N, r.s.K, r.s.V, r.s.B, d_levels, r.w.dist, d_R, d_O, d_E, d_theta, sigma,
                     r.w.opart);
  hipLaunchKernelGGL(k_hm_obj_finish, dim3(1), dim3(256), 0, r.st, (int64_t)hm_cells(N), r.w.opart, d_obj);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_harmony_correct_device(gficf_ctx* ctx, int64_t N, int64_t d, int64_t K, int64_t V, int64_t B, const int32_t* var_start,
                                 const double* d_Z, const int32_t* d_levels, const double* d_R, const double* d_lambda, double* d_Zcorr,
                                 double* d_W, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  HmRun r;
  if (!var_start) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL var_start");
  GFICF_RC(hm_enter(r, ctx, N, d, K, V, B, var_start, ws, ws_bytes));
  if (!d_Z || !d_levels || !d_R || !d_lambda || !d_Zcorr) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  const HmShape& s = r.s;
  const int64_t nbx = r.bx.start[r.bx.nv];
  GFICF_HIP_CHECK(hipMemsetAsync(r.w.status + 1, 0, sizeof(uint32_t), r.st));
  hipLaunchKernelGGL(k_hm_levels, dim3(hm_cells(N)), dim3(256), 0, r.st, N, r.bx, d_levels, r.w.ext, r.w.status);
  hm_binsum(r, N, nullptr, d_R, r.w.ext, r.bx, r.w.bpart);
  hipLaunchKernelGGL(k_hm_sumparts, dim3(hm_cells(K * nbx)), dim3(256), 0, r.st, s.nch, K * nbx, r.w.bpart, r.w.Q);
  hipLaunchKernelGGL(k_hm_moment_part, dim3((unsigned)s.nchm, s.K, (unsigned)gficf_ceil_div(s.B, s.bt)), dim3(s.LJ), 0, r.st, N, s.d, s.K, s.V, s.B, s.chm,
                     s.bt, d_Z, d_R, r.w.ext, r.w.mpart);
  hipLaunchKernelGGL(k_hm_sumparts, dim3(hm_cells(K * B * d)), dim3(256), 0, r.st, s.nchm, K * B * d, r.w.mpart, r.w.M);
  hipLaunchKernelGGL(k_hm_solve, dim3(s.K), dim3(256), 0, r.st, s.d, s.B, r.bx, r.w.Q, r.w.M, d_lambda, r.w.W, r.w.status);
  hipLaunchKernelGGL(k_hm_apply, dim3((unsigned)gficf_ceil_div(N, 256 / s.LJ)), dim3(256), 0, r.st, N, s.d, s.K, s.V, s.B, s.LJ, d_Z, r.w.ext, d_R, r.w.W,
                     d_Zcorr);
  if (d_W) GFICF_HIP_CHECK(hipMemcpyAsync(d_W, r.w.W, sizeof(double) * (size_t)(K * (B + 1) * d), hipMemcpyDeviceToDevice, r.st));
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_harmony_device(gficf_ctx* ctx, int64_t N, int64_t d, int64_t K, int64_t V, int64_t B, const int32_t* var_start, const double* d_Z,
                         const int32_t* d_levels, const double* d_theta, const double* d_lambda, double sigma, const double* d_Y0,
                         const int32_t* d_perm, int64_t rounds, int32_t init_iter, int32_t max_iter_harmony, int32_t max_iter_kmeans,
                         int32_t n_blocks, double epsilon_cluster, double epsilon_harmony, double* d_Zcorr, double* d_Zc, double* d_R,
                         double* d_Y, double* d_O, double* d_E, double* objective, int32_t* iter_rounds, int64_t* info, void* ws,
                         size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  HmRun r;
  if (!var_start) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL var_start");
  GFICF_RC(hm_enter(r, ctx, N, d, K, V, B, var_start, ws, ws_bytes));
  GFICF_RC(hm_sigma(sigma));
  if (init_iter < 0 || max_iter_harmony < 0 || max_iter_kmeans < 0 || n_blocks < 1)
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "init_iter = %d, max_iter_harmony = %d, max_iter_kmeans = %d, n_blocks = %d: a limit is out of range", (int)init_iter,
               (int)max_iter_harmony, (int)max_iter_kmeans, (int)n_blocks);
  if (rounds < (int64_t)max_iter_harmony * max_iter_kmeans)
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "perm has %lld rounds, %lld may be run", (long long)rounds, (long long)max_iter_harmony * max_iter_kmeans);
  if (!d_Z || !d_levels || !d_theta || !d_lambda || !d_Y0 || (rounds > 0 && !d_perm) || !d_Zcorr || !d_Zc || !d_R || !d_Y || !d_O || !d_E || !objective ||
      !iter_rounds || !info)
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  auto read_obj = [&](double* out) -> int {
    GFICF_RC(gficf_harmony_objective_device(ctx, N, d, K, V, B, var_start, d_Zc, d_levels, d_Y, d_R, d_O, d_E, d_theta, sigma, r.w.obj, ws, ws_bytes));
    GFICF_HIP_CHECK(hipMemcpyAsync(out, r.w.obj, sizeof(double), hipMemcpyDeviceToHost, r.st));
    GFICF_HIP_CHECK(hipStreamSynchronize(r.st));
    return GFICF_OK;
  };
  GFICF_RC(gficf_harmony_normalise_device(ctx, N, d, d_Z, d_Zc, ws, ws_bytes));
  GFICF_RC(gficf_harmony_start_device(ctx, N, d, K, d_Zc, d_Y0, init_iter, d_Y, r.w.lab, ws, ws_bytes));
  GFICF_RC(gficf_harmony_assign_device(ctx, N, d, K, V, B, var_start, d_Zc, d_levels, d_Y, sigma, d_R, d_O, d_E, ws, ws_bytes));
  GFICF_HIP_CHECK(hipMemcpyAsync(d_Zcorr, d_Z, sizeof(double) * (size_t)(N * d), hipMemcpyDeviceToDevice, r.st));
  int64_t n_obj = 0, used = 0, iters = 0, converged = 0;
  GFICF_RC(read_obj(objective + n_obj));
  ++n_obj;
  double h_prev = 0.0;
  for (int it = 1; it <= max_iter_harmony; ++it) {
    int t = 0;
    while (t < max_iter_kmeans) {
      GFICF_RC(gficf_harmony_round_device(ctx, N, d, K, V, B, var_start, d_Zc, d_levels, d_theta, sigma, d_perm + used * N, n_blocks, d_R, d_O, d_E, d_Y,
                                          ws, ws_bytes));
      ++used;
      ++t;
      GFICF_RC(read_obj(objective + n_obj));
      ++n_obj;
      if (t >= 3) {
        const double* o = objective + n_obj;
        const double older = o[-4] + o[-3] + o[-2], newer = o[-3] + o[-2] + o[-1];
        if ((older - newer) / fabs(older) < epsilon_cluster) break;
      }
    }
    iter_rounds[it - 1] = t;
    GFICF_RC(gficf_harmony_correct_device(ctx, N, d, K, V, B, var_start, d_Z, d_levels, d_R, d_lambda, d_Zcorr, nullptr, ws, ws_bytes));
    // the normalisation keeps the counters of the run: only its own zero-row count starts again
    GFICF_HIP_CHECK(hipMemsetAsync(r.w.status + 2, 0, sizeof(uint32_t), r.st));
    hipLaunchKernelGGL(k_hm_normalise, dim3(hm_cells(N)), dim3(256), 0, r.st, N, (int)d, d_Zcorr, d_Zc, r.w.status);
    GFICF_HIP_CHECK(hipGetLastError());
    iters = it;
    const double h = objective[n_obj - 1];
    if (it >= 2 && (h_prev - h) / fabs(h_prev) < epsilon_harmony) { converged = 1; break; }
    h_prev = h;
  }
  info[0] = iters; info[1] = used; info[2] = converged; info[3] = 0;
  return GFICF_OK;
}

int gficf_harmony_sync(gficf_ctx* ctx, const void* ws, int64_t* info) {
  GFICF_CTX_ENTER(ctx);
  if (!ws) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL workspace");
  uint32_t st[4] = {0, 0, 0, 0};
  GFICF_HIP_CHECK(hipMemcpyAsync(st, ws, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  GFICF_RC(gficf_ctx_sync(ctx));
  if (info) { info[0] = st[2]; info[1] = st[1]; }
  if (st[0] & HM_ST_LEVEL) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a level id outside its variable's range");
  if (st[0] & HM_ST_PERM) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "an entry of perm outside [0, N)");
  if (st[0] & HM_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "a row of Z whose norm is not finite");
  return GFICF_OK;
}

}  // extern "C"
