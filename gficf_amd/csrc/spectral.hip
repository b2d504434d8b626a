// spectral.hip — connected components of a CSR graph and the leading eigenvectors of its normalised Laplacian (uwot's spectral
// initialisation of UMAP).  Built into libgficf_spectral.so, which links libgficf_hip.so and uses its context, pool and error
// plumbing (include/gficf_spectral.h states the contract, the method and every threshold).
//
// Launches of the components entry (N vertices):
//   k_cc_check       one lane per row: the row pointers and the columns checked, parent[i] = i
//   per round        k_cc_hook (8 lanes per row: atomicMin of the larger parent by the smaller), k_cc_jump (one lane per vertex:
//                    its parent becomes its root); one word read back
//   k_cc_count, k_cc_info   the roots counted (an integer counter), the info block written
// Launches of the solve (b = ndim columns per block, at most m basis columns, SP_RED = 128 fixed row chunks):
//   once             k_sp_degree, the norm of sqrt(d) (k_sp_proj_part + k_sp_q0), k_sp_hubs
//   per block        k_sp_mul<b>                       W = S V_j, from the pre-scaled block Xs = D^-1/2 V_j
//                    2 x (k_sp_proj_part, k_sp_proj_fin, k_sp_axpy<b>)   c = [q0 V]' W over the chunks, their sum in order, W -= [q0 V] c
//                    2 x (k_sp_proj_part, k_sp_chol, k_sp_apply<b>)      G = W' W, the b x b kernel, W <- W T; the second writes V_{j+1} and Xs
//   per cycle        blocks until the next would not fit: capped by m the cycle ends at its last FULL block (me <= mc columns, no column
//                    of a remainder discarded), capped by N - 1 the last block is as narrow as what is left; G_last = W_last' W_last
//   per restart      k_sp_rotate (V <- V Z, over the me columns of the cycle; Z: the kept Ritz vectors, chosen on the host), k_sp_apply<b> (the residual block W_last Z_last)
//   at the end       k_sp_rotate, k_sp_amax_part / k_sp_sign_fin / k_sp_flip (the sign rule), k_sp_scale, k_sp_mul<b>, k_sp_resid<b>, the norms
// The solve is one SpRun, its steps named after the rows above: prepare (once), start, then per cycle grow, read_cycle (the cycle's
// one synchronisation), ritz, finish (at the end: when the estimate passes or nothing is left to restart with), else restart;
// sp_solve is that loop.  What the host computes between a read-back and the next upload (Rayleigh-Ritz by cyclic Jacobi, the
// estimate, the final rotation, which Ritz vectors a restart keeps) is spectral_ritz.h: no GPU header, tested on the CPU.
// What bounds a block step at 54 000 vertices: P (12 B an entry) and V (N x m f64) both stay in the L2 / the infinity cache, the
// kernels are short, so the step is about thirteen launch latencies.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include "addon_status.h"
#include "common.h"
#include "gficf_spectral.h"
#include "spectral_ritz.h"

namespace {

constexpr int SP_RED = 128;                  // fixed chunks of a reduction (one workgroup each)
constexpr int SP_HUB_LEN = 256;              // a row longer than this is multiplied by a whole wave
constexpr int SP_GROUP = 8;                  // lanes per row otherwise
constexpr int SP_HUB_WAVES = 1024;           // waves that share the hub list, at most
constexpr int SP_MAXB = GFICF_SPECTRAL_MAX_NDIM;
constexpr uint32_t SP_ST_ID = GFICF_AST_ID;          // a column outside [0, N)
constexpr uint32_t SP_ST_VALUE = GFICF_AST_VALUE;    // a value of P that is not positive and finite
constexpr uint32_t SP_ST_CSC = GFICF_AST_CSC;        // a row pointer that does not start at 0, decreases or leaves [0, capacity]

unsigned sp_grid(int64_t n) { return (unsigned)gficf_ceil_div(n > 0 ? n : 1, 256); }

// ------------------------------------------------------------------------------------------------ components
__global__ __launch_bounds__(256) void k_cc_check(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N, int64_t cap,
                                                  int32_t* __restrict__ parent, uint32_t* __restrict__ status) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= N) return;
  parent[v] = (int32_t)v;
  const int64_t b = rowptr[v], e = rowptr[v + 1];
  if (b < 0 || e < b || e > cap || (v == 0 && b != 0)) {
    atomicOr(status, SP_ST_CSC);
    return;
  }
  bool bad = false;
  for (int64_t t = b; t < e; ++t) {
    const int32_t j = col[t];
    bad |= j < 0 || (int64_t)j >= N;
  }
  if (bad) atomicOr(status, SP_ST_ID);
}

// (checked rows and columns only: the entry returns before this launch otherwise)
__global__ __launch_bounds__(256) void k_cc_hook(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N, int32_t* parent,
                                                 uint32_t* __restrict__ changed) {
  const int64_t v = (int64_t)blockIdx.x * (256 / SP_GROUP) + threadIdx.x / SP_GROUP;
  if (v >= N) return;
  const int lane = threadIdx.x & (SP_GROUP - 1);
  const int64_t e1 = rowptr[v + 1];
  bool any = false;
  for (int64_t e = rowptr[v] + lane; e < e1; e += SP_GROUP) {
    const int32_t pu = parent[v], pw = parent[col[e]];
    if (pu == pw) continue;
    const int32_t lo = pu < pw ? pu : pw, hi = pu < pw ? pw : pu;
    any |= atomicMin(parent + hi, lo) > lo;
  }
  if (any) atomicOr(changed, 1u);
}

__global__ __launch_bounds__(256) void k_cc_jump(int64_t N, int32_t* parent) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= N) return;
  int32_t p = parent[v];
  for (int32_t g = parent[p]; g != p; g = parent[p]) p = g;     // parents only ever decrease: the chain ends at a root
  parent[v] = p;
}

__global__ __launch_bounds__(256) void k_cc_count(int64_t N, const int32_t* __restrict__ parent, uint32_t* __restrict__ count) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool root = v < N && (int64_t)parent[v] == v;
  const unsigned long long m = __ballot(root);
  if (m && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(m)) atomicAdd(count, (uint32_t)__builtin_popcountll(m));
}

__global__ void k_cc_info(const uint32_t* __restrict__ count, int64_t rounds, int64_t* __restrict__ info) {
  info[0] = (int64_t)*count;
  info[1] = rounds;
}

struct CcWs {
  uint32_t *status, *changed, *count;
};

size_t cc_carve(char* base, CcWs& w) {
  gficf_carver cv;
  cv.base = base;
  w.status = cv.take<uint32_t>(1);
  w.changed = cv.take<uint32_t>(1);
  w.count = cv.take<uint32_t>(1);
  return cv.total();
}

// the components of a graph into d_labels; *comps and *rounds on the host.  Synchronises.
int cc_run(gficf_ctx* ctx, const CcWs& w, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, int64_t cap, int32_t* d_labels, int64_t* d_info,
           int64_t* comps, int64_t* rounds) {
  hipStream_t st = ctx->stream;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.count, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_cc_check, dim3(sp_grid(N)), dim3(256), 0, st, d_rowptr, d_col, N, cap, d_labels, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  uint32_t h = 0;
  GFICF_HIP_CHECK(hipMemcpyAsync(&h, w.status, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  GFICF_HIP_CHECK(hipStreamSynchronize(st));
  if (h & SP_ST_CSC) GFICF_FAIL(GFICF_ERR_BAD_CSC, "a row pointer of the graph does not start at 0, decreases or leaves [0, capacity]");
  if (h & SP_ST_ID) GFICF_FAIL(GFICF_ERR_BAD_ID, "a column of the graph outside [0, N)");
  int64_t r = 0;
  for (;;) {
    GFICF_HIP_CHECK(hipMemsetAsync(w.changed, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_cc_hook, dim3((unsigned)gficf_ceil_div(N, 256 / SP_GROUP)), dim3(256), 0, st, d_rowptr, d_col, N, d_labels, w.changed);
    hipLaunchKernelGGL(k_cc_jump, dim3(sp_grid(N)), dim3(256), 0, st, N, d_labels);
    GFICF_HIP_CHECK(hipGetLastError());
    GFICF_HIP_CHECK(hipMemcpyAsync(&h, w.changed, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GFICF_HIP_CHECK(hipStreamSynchronize(st));
    ++r;
    if (!h || r > N) break;                                     // (r > N cannot happen: a round that hooks removes a tree)
  }
  uint32_t c = 0;
  hipLaunchKernelGGL(k_cc_count, dim3(sp_grid(N)), dim3(256), 0, st, N, (const int32_t*)d_labels, w.count);
  if (d_info) hipLaunchKernelGGL(k_cc_info, dim3(1), dim3(1), 0, st, (const uint32_t*)w.count, r, d_info);
  GFICF_HIP_CHECK(hipGetLastError());
  GFICF_HIP_CHECK(hipMemcpyAsync(&c, w.count, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  GFICF_HIP_CHECK(hipStreamSynchronize(st));
  *comps = (int64_t)c;
  *rounds = r;
  return GFICF_OK;
}

// ------------------------------------------------------------------------------------------------ solve: degree, q0, hubs
__global__ __launch_bounds__(256) void k_sp_degree(const int64_t* __restrict__ rowptr, const float* __restrict__ val, int64_t N, double* __restrict__ sq,
                                                   double* __restrict__ dis, uint32_t* __restrict__ status) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= N) return;
  double d = 0.0;
  bool bad = false;
  for (int64_t e = rowptr[v]; e < rowptr[v + 1]; ++e) {         // column order
    const float w = val[e];
    bad |= !(w > 0.f) || isinf(w);
    d += (double)w;
  }
  if (bad) atomicOr(status, SP_ST_VALUE);
  sq[v] = sqrt(d);
  dis[v] = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
}

__global__ __launch_bounds__(256) void k_sp_q0(const double* __restrict__ parts, int64_t N, double* __restrict__ q0) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= N) return;
  double s = 0.0;
  for (int c = 0; c < SP_RED; ++c) s += parts[c];
  q0[v] = q0[v] / sqrt(s);
}

__global__ __launch_bounds__(256) void k_sp_hubs(const int64_t* __restrict__ rowptr, int64_t N, int32_t* __restrict__ hubs, uint32_t hub_cap,
                                                 uint32_t* __restrict__ nhubs) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= N) return;
  if (rowptr[v + 1] - rowptr[v] > SP_HUB_LEN) {
    const uint32_t at = atomicAdd(nhubs, 1u);                   // the list's order is free: a wave takes a whole row
    if (at < hub_cap) hubs[at] = (int32_t)v;
  }
}

// ------------------------------------------------------------------------------------------------ solve: W = S X
struct SpMul {
  int64_t N;
  const int64_t* rowptr;
  const int32_t* col;
  const float* val;
  const double* dis;
  const int32_t* hubs;
  const uint32_t* nhubs;
  uint32_t hub_cap;
};

// row v by the G lanes lane0 .. lane0 + G - 1 of a wave: lane l adds entries l, l + G, ... in order, the lanes' sums by a butterfly
template <int B, int G>
__device__ inline void sp_row(const SpMul& L, int64_t v, const double* __restrict__ Xs, double* __restrict__ W) {
  const int lane = (threadIdx.x & 63) & (G - 1);
  const int64_t e1 = L.rowptr[v + 1];
  double acc[B];
#pragma unroll
  for (int c = 0; c < B; ++c) acc[c] = 0.0;
  for (int64_t e = L.rowptr[v] + lane; e < e1; e += G) {
    const double w = (double)L.val[e];
    const double* x = Xs + (int64_t)L.col[e] * B;
    if (B % 2 == 0) {
#pragma unroll
      for (int c = 0; c < B; c += 2) {
        const double2 p = *reinterpret_cast<const double2*>(x + c);   // 16 B: both columns of a neighbour at b = 2
        acc[c] += w * p.x;
        acc[c + 1 < B ? c + 1 : c] += w * p.y;
      }
    } else {
#pragma unroll
      for (int c = 0; c < B; ++c) acc[c] += w * x[c];
    }
  }
#pragma unroll
  for (int c = 0; c < B; ++c) {
#pragma unroll
    for (int d = G / 2; d >= 1; d >>= 1) acc[c] += __shfl_xor(acc[c], d, G);
  }
  if (lane == 0) {
    const double s = L.dis[v];
#pragma unroll
    for (int c = 0; c < B; ++c) W[v * B + c] = s * acc[c];
  }
}

template <int B>
__global__ __launch_bounds__(256) void k_sp_mul(SpMul L, unsigned vertex_blocks, const double* __restrict__ Xs, double* __restrict__ W) {
  if (blockIdx.x < vertex_blocks) {
    const int64_t v = (int64_t)blockIdx.x * (256 / SP_GROUP) + threadIdx.x / SP_GROUP;
    if (v >= L.N) return;
    if (L.rowptr[v + 1] - L.rowptr[v] > SP_HUB_LEN) return;     // a wave of the blocks behind takes it
    sp_row<B, SP_GROUP>(L, v, Xs, W);
  } else {
    const uint32_t waves = (gridDim.x - vertex_blocks) * 4u, wave = (blockIdx.x - vertex_blocks) * 4u + threadIdx.x / 64u;
    uint32_t nh = *L.nhubs;
    if (nh > L.hub_cap) nh = L.hub_cap;
    for (uint32_t h = wave; h < nh; h += waves) sp_row<B, 64>(L, (int64_t)L.hubs[h], Xs, W);
  }
}

// ------------------------------------------------------------------------------------------------ solve: tall-skinny products
// out (jj, c) = sum over the rows of chunk blockIdx.x of A[r, jj] W[r, c], jj < na (and jj = na: q0, when given); n_out = rows x b.
// 256 / n_out sub-groups deal the chunk's rows round robin, their sums are added in order: a fixed order for fixed N, na, b.
__global__ __launch_bounds__(256) void k_sp_proj_part(const double* __restrict__ A, int lda, int na, const double* __restrict__ q0,
                                                      const double* __restrict__ W, int b, int64_t N, double* __restrict__ parts) {
  __shared__ double sh[256];
  const int n_out = (na + (q0 ? 1 : 0)) * b, t = threadIdx.x;
  const int64_t per = gficf_ceil_div(N, SP_RED), lo = (int64_t)blockIdx.x * per, hi = lo + per < N ? lo + per : N;
  for (int o0 = 0; o0 < n_out; o0 += 256) {
    const int cnt = n_out - o0 < 256 ? n_out - o0 : 256, nsub = 256 / cnt;
    const int sub = t / cnt, o = o0 + t - sub * cnt, jj = o / b, c = o - jj * b;
    double s = 0.0;
    if (sub < nsub) {
      if (jj < na) {
        for (int64_t r = lo + sub; r < hi; r += nsub) s += A[r * lda + jj] * W[r * b + c];
      } else {
        for (int64_t r = lo + sub; r < hi; r += nsub) s += q0[r] * W[r * b + c];
      }
    }
    sh[t] = s;
    __syncthreads();
    if (t < cnt) {
      double a = 0.0;
      for (int u = 0; u < nsub; ++u) a += sh[u * cnt + t];
      parts[(int64_t)blockIdx.x * n_out + o0 + t] = a;
    }
    __syncthreads();
  }
}

// the chunks added in order: C (n_out).  With Hcol: column c of the block gets C (pass 0) or has it added (pass 1), rows < na;
// with nb: the squared norm of every column of C likewise (what the projection took out of W)
__global__ __launch_bounds__(256) void k_sp_proj_fin(const double* __restrict__ parts, int n_out, double* __restrict__ C, double* __restrict__ Hcol,
                                                     int ldh, int na, int b, double* __restrict__ nb, int pass) {
  for (int o = threadIdx.x; o < n_out; o += 256) {
    double s = 0.0;
    for (int ch = 0; ch < SP_RED; ++ch) s += parts[(int64_t)ch * n_out + o];
    C[o] = s;
    const int jj = o / b, c = o - jj * b;
    if (Hcol && jj < na) {
      if (pass == 0) Hcol[jj + (int64_t)ldh * c] = s;
      else Hcol[jj + (int64_t)ldh * c] += s;
    }
  }
  __syncthreads();
  if (nb && (int)threadIdx.x < b) {
    double s = 0.0;
    for (int jj = 0; jj * b < n_out; ++jj) s += C[jj * b + threadIdx.x] * C[jj * b + threadIdx.x];
    nb[threadIdx.x] = pass == 0 ? s : nb[threadIdx.x] + s;
  }
}

template <int B>
__global__ __launch_bounds__(256) void k_sp_axpy(const double* __restrict__ A, int lda, int na, const double* __restrict__ q0,
                                                 const double* __restrict__ C, double* __restrict__ W, int64_t N) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  double acc[B];
#pragma unroll
  for (int c = 0; c < B; ++c) acc[c] = 0.0;
  for (int jj = 0; jj < na; ++jj) {
    const double a = A[r * lda + jj];
#pragma unroll
    for (int c = 0; c < B; ++c) acc[c] += a * C[jj * B + c];
  }
  if (q0) {
    const double a = q0[r];
#pragma unroll
    for (int c = 0; c < B; ++c) acc[c] += a * C[na * B + c];
  }
#pragma unroll
  for (int c = 0; c < B; ++c) W[r * B + c] -= acc[c];
}

// ------------------------------------------------------------------------------------------------ solve: the b x b work
// G = the chunks of W' W added in order; T (b x b, T[k b + j]) with W T orthonormal: Gram-Schmidt in the G inner product, column by
// column.  Dropped (a zero column of T): a column >= bw; on the first of the two passes one whose squared norm G_jj is <= 1e-24 x
// the one before the projection (nb_j + G_jj); a pivot <= 1e-12 G_jj.  alive (given on the second pass): one flag per column < bw.
__global__ __launch_bounds__(64) void k_sp_chol(const double* __restrict__ parts, int b, int bw, int first, const double* __restrict__ nb,
                                                double* __restrict__ T, int32_t* __restrict__ alive) {
  __shared__ double G[SP_MAXB * SP_MAXB], Ts[SP_MAXB * SP_MAXB], tj[SP_MAXB];
  const int t = threadIdx.x;
  if (t < b * b) {
    double s = 0.0;
    for (int ch = 0; ch < SP_RED; ++ch) s += parts[ch * b * b + t];
    G[t] = s;
    Ts[t] = 0.0;
  }
  __syncthreads();
  if (t != 0) return;
  for (int j = 0; j < b; ++j) {
    const double gjj = G[j * b + j];
    bool dead = j >= bw;
    if (!dead) dead = first ? !(gjj > 1e-24 * (nb[j] + gjj)) : !(gjj > 0.0);
    double n2 = 0.0;
    if (!dead) {
      for (int k = 0; k < b; ++k) tj[k] = k == j ? 1.0 : 0.0;
      for (int i = 0; i < j; ++i) {                             // (a dropped column i is zero: it takes nothing)
        double s = 0.0;
        for (int k = 0; k < b; ++k) s += Ts[k * b + i] * G[k * b + j];
        for (int k = 0; k < b; ++k) tj[k] -= s * Ts[k * b + i];
      }
      for (int k = 0; k < b; ++k) {
        double s = 0.0;
        for (int l = 0; l < b; ++l) s += G[k * b + l] * tj[l];
        n2 += tj[k] * s;
      }
      dead = !(n2 > 1e-12 * gjj);
    }
    const double inv = dead ? 0.0 : 1.0 / sqrt(n2);
    for (int k = 0; k < b; ++k) Ts[k * b + j] = dead ? 0.0 : tj[k] * inv;
    if (alive && j < bw) alive[j] = dead ? 0 : 1;
  }
  for (int k = 0; k < b * b; ++k) T[k] = Ts[k];
}

// W <- W T, row by row.  With V: the first bw columns also become columns col0 .. of V, and Xs = D^-1/2 W the next multiplicand.
template <int B>
__global__ __launch_bounds__(256) void k_sp_apply(double* __restrict__ W, const double* __restrict__ T, int64_t N, double* __restrict__ V, int ldv,
                                                  int col0, int bw, double* __restrict__ Xs, const double* __restrict__ dis) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  double w[B], o[B];
#pragma unroll
  for (int c = 0; c < B; ++c) { w[c] = W[r * B + c]; o[c] = 0.0; }
#pragma unroll
  for (int k = 0; k < B; ++k) {
#pragma unroll
    for (int c = 0; c < B; ++c) o[c] += w[k] * T[k * B + c];
  }
#pragma unroll
  for (int c = 0; c < B; ++c) W[r * B + c] = o[c];
  if (V) {
    const double s = dis[r];
#pragma unroll
    for (int c = 0; c < B; ++c) {
      if (c < bw) V[r * ldv + col0 + c] = o[c];
      Xs[r * B + c] = c < bw ? s * o[c] : 0.0;
    }
  }
}

// out[r, l] = sum_j Vin[r, j] Z[j kp + l], j < mc in order; one lane per (r, l)
__global__ __launch_bounds__(256) void k_sp_rotate(const double* __restrict__ Vin, int ldv, int mc, const double* __restrict__ Z, int kp,
                                                   double* __restrict__ out, int ldo, int64_t N) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= N * kp) return;
  const int64_t r = t / kp;
  const int l = (int)(t - r * kp);
  double s = 0.0;
  for (int j = 0; j < mc; ++j) s += Vin[r * ldv + j] * Z[j * kp + l];
  out[r * ldo + l] = s;
}

// ------------------------------------------------------------------------------------------------ solve: sign rule, residuals
__global__ __launch_bounds__(64) void k_sp_amax_part(const double* __restrict__ X, int b, int64_t N, double* __restrict__ pv, int64_t* __restrict__ pi) {
  const int c = threadIdx.x;
  if (c >= b) return;
  const int64_t per = gficf_ceil_div(N, SP_RED), lo = (int64_t)blockIdx.x * per, hi = lo + per < N ? lo + per : N;
  double best = -1.0;
  int64_t at = -1;
  for (int64_t r = lo; r < hi; ++r) {
    const double a = fabs(X[r * b + c]);
    if (a > best) { best = a; at = r; }                         // strict: the lowest index on ties
  }
  pv[blockIdx.x * b + c] = best;
  pi[blockIdx.x * b + c] = at;
}

__global__ __launch_bounds__(64) void k_sp_sign_fin(const double* __restrict__ X, int b, const double* __restrict__ pv, const int64_t* __restrict__ pi,
                                                    double* __restrict__ sign) {
  const int c = threadIdx.x;
  if (c >= b) return;
  double best = -1.0;
  int64_t at = -1;
  for (int ch = 0; ch < SP_RED; ++ch)
    if (pv[ch * b + c] > best) { best = pv[ch * b + c]; at = pi[ch * b + c]; }
  sign[c] = (at >= 0 && X[at * b + c] < 0.0) ? -1.0 : 1.0;
}

// X *= sign (column-wise); Xs = D^-1/2 X
__global__ __launch_bounds__(256) void k_sp_flip_scale(double* __restrict__ X, int b, int64_t N, const double* __restrict__ sign,
                                                       const double* __restrict__ dis, double* __restrict__ Xs) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= N * b) return;
  const int64_t r = t / b;
  const double x = X[t] * sign[t - r * b];
  X[t] = x;
  Xs[t] = dis[r] * x;
}

template <int B>
__global__ __launch_bounds__(256) void k_sp_resid(double* __restrict__ W, const double* __restrict__ X, const double* __restrict__ theta, int64_t N) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
#pragma unroll
  for (int c = 0; c < B; ++c) W[r * B + c] -= theta[c] * X[r * B + c];
}

// the one place that knows for which block widths the templated kernels exist: fn(std::integral_constant<int, B>{}), default: 8
template <typename F>
void with_block_width(int b, F&& fn) {
  switch (b) {
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 3: return fn(std::integral_constant<int, 3>{});
    case 4: return fn(std::integral_constant<int, 4>{});
    case 5: return fn(std::integral_constant<int, 5>{});
    case 6: return fn(std::integral_constant<int, 6>{});
    case 7: return fn(std::integral_constant<int, 7>{});
    default: return fn(std::integral_constant<int, 8>{});
  }
}

// ------------------------------------------------------------------------------------------------ solve: workspace
struct SpWs {
  CcWs cc;
  int32_t* labels;
  int64_t* ccinfo;
  double *q0, *dis, *Va, *Vb, *W, *Xs, *Wf, *Xfs, *parts, *C, *H, *nb, *G, *T, *Z, *Zl, *theta, *sign, *pv;
  int64_t* pi;
  int32_t* flags;
  uint32_t* nhubs;
  int32_t* hubs;
  uint32_t hub_cap;
  int ldh;
};

size_t sp_carve(char* base, int64_t N, int64_t cap, int b, int m, SpWs& w) {
  gficf_carver cv;
  cv.base = base;
  const size_t n = (size_t)N, nb = n * (size_t)b;
  char* cc = cv.take<char>(cc_carve(nullptr, w.cc));
  cc_carve(cc, w.cc);
  w.labels = cv.take<int32_t>(n);
  w.ccinfo = cv.take<int64_t>(2);
  w.q0 = cv.take<double>(n);
  w.dis = cv.take<double>(n);
  w.Va = cv.take<double>(n * (size_t)m);
  w.Vb = cv.take<double>(n * (size_t)m);
  w.W = cv.take<double>(nb);
  w.Xs = cv.take<double>(nb);
  w.Wf = cv.take<double>(nb);
  w.Xfs = cv.take<double>(nb);
  w.parts = cv.take<double>((size_t)SP_RED * (size_t)(m + 1) * (size_t)b);
  w.C = cv.take<double>((size_t)(m + 1) * (size_t)b);
  w.ldh = m;
  w.H = cv.take<double>((size_t)m * (size_t)(m + SP_MAXB));   // a block's columns past the last basis column are written too
  w.nb = cv.take<double>(SP_MAXB);
  w.G = cv.take<double>(SP_MAXB * SP_MAXB);
  w.T = cv.take<double>(SP_MAXB * SP_MAXB);
  w.Z = cv.take<double>((size_t)m * (size_t)(SP_MAXB + 2));
  w.Zl = cv.take<double>(SP_MAXB * SP_MAXB);
  w.theta = cv.take<double>(SP_MAXB);
  w.sign = cv.take<double>(SP_MAXB);
  w.pv = cv.take<double>((size_t)SP_RED * SP_MAXB);
  w.pi = cv.take<int64_t>((size_t)SP_RED * SP_MAXB);
  w.flags = cv.take<int32_t>((size_t)m + SP_MAXB);
  w.nhubs = cv.take<uint32_t>(1);
  w.hub_cap = (uint32_t)(cap / SP_HUB_LEN + 1);
  w.hubs = cv.take<int32_t>(w.hub_cap);
  return cv.total();
}

int sp_check(int64_t N, int64_t cap, int ndim, double tol, int m, int max_restarts) {
  if (N < 1 || N > 0x7FFFFFFFll) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld outside [1, 2^31)", (long long)N);
  if (cap < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative capacity");
  if (ndim < 1 || ndim > GFICF_SPECTRAL_MAX_NDIM) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ndim = %d outside [1, %d]", ndim, GFICF_SPECTRAL_MAX_NDIM);
  if (N <= (int64_t)ndim) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld vertices for ndim = %d: N must exceed ndim", (long long)N, ndim);
  if (m < 2 * ndim + 2 || m > GFICF_SPECTRAL_MAX_M)
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "m = %d outside [2 ndim + 2, %d] = [%d, %d]", m, GFICF_SPECTRAL_MAX_M, 2 * ndim + 2, GFICF_SPECTRAL_MAX_M);
  if (!(tol > 0.0) || !std::isfinite(tol)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "tol = %g must be positive and finite", tol);
  if (max_restarts < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "max_restarts = %d", max_restarts);
  return GFICF_OK;
}

// a caller's workspace carved: carve(base) takes the pieces from base on and returns their total; base == nullptr only counts
template <typename F>
int sp_take(void* ws, size_t ws_bytes, F&& carve) {
  const size_t need = carve((char*)nullptr);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  carve((char*)ws);
  return GFICF_OK;
}

// ------------------------------------------------------------------------------------------------ solve: the run
// One solve on a carved workspace, one component known; sp_solve below drives its steps.  The host mathematics between a cycle's
// read-back and the next upload is spectral_ritz.h's.  What an asynchronous upload reads (rz.theta, zb, rs.up, rs.zl) lives here
// and is written only right behind a synchronisation: untouched until the next one.
struct SpRun {
  gficf_ctx* ctx;
  hipStream_t st;
  SpWs w;
  int64_t N;
  int b, m, mc, ldv, ldh, max_restarts;
  bool capped;                                                  // by m, not by the complement of q0
  double tol;
  SpMul L;
  unsigned vb;                                                  // the multiply's grid: vb blocks of vertices, then the waves of the hub list
  dim3 mulgrid, rows, one{1}, red{SP_RED};
  double *V, *Vo;                                               // the basis, and where a restart rotates it to
  int64_t mults = 0;
  int restarts = 0, converged = 0;
  int c0 = 0, bw = 0, nc = 0, keep = 0;                         // the last block's first column and width, the columns so far, the kept ones
  std::vector<double> hH, hG, hres, zb, resid;                  // read back: H, G_last, the residual Gram matrix; Z[:, :b]; the residual norms
  std::vector<int32_t> hflags;
  SpRitz rz;
  SpRestart rs;

  SpRun(gficf_ctx* c, const SpWs& ws, int64_t n, const int64_t* rowptr, const int32_t* col, const float* val, int b_, double tol_, int m_, int mr)
      : ctx(c), st(c->stream), w(ws), N(n), b(b_), m(m_), mc((int64_t)m_ < n - 1 ? m_ : (int)(n - 1)), ldv(m_), ldh(ws.ldh), max_restarts(mr),
        capped((int64_t)mc < n - 1), tol(tol_), L{n, rowptr, col, val, ws.dis, ws.hubs, ws.nhubs, ws.hub_cap},
        vb((unsigned)gficf_ceil_div(n, 256 / SP_GROUP)), rows(sp_grid(n)), V(ws.Va), Vo(ws.Vb), hH((size_t)ldh * (size_t)m_), hG((size_t)b_ * b_),
        hres((size_t)b_ * b_), resid((size_t)b_, 0.0), hflags((size_t)m_) {
    const int64_t hw = w.hub_cap < (uint32_t)SP_HUB_WAVES ? (int64_t)w.hub_cap : (int64_t)SP_HUB_WAVES;
    mulgrid = dim3(vb + (unsigned)gficf_ceil_div(hw, 4));
  }

  // the degrees, q0 = sqrt(d) / |sqrt(d)|, the hub list
  int prepare() {
    GFICF_HIP_CHECK(hipMemsetAsync(w.cc.status, 0, sizeof(uint32_t), st));
    GFICF_HIP_CHECK(hipMemsetAsync(w.nhubs, 0, sizeof(uint32_t), st));
    GFICF_HIP_CHECK(hipMemsetAsync(w.H, 0, sizeof(double) * (size_t)ldh * (size_t)(m + SP_MAXB), st));
    hipLaunchKernelGGL(k_sp_degree, rows, dim3(256), 0, st, L.rowptr, L.val, N, w.q0, w.dis, w.cc.status);
    hipLaunchKernelGGL(k_sp_proj_part, red, dim3(256), 0, st, (const double*)w.q0, 1, 1, (const double*)nullptr, (const double*)w.q0, 1, N, w.parts);
    hipLaunchKernelGGL(k_sp_q0, rows, dim3(256), 0, st, (const double*)w.parts, N, w.q0);
    hipLaunchKernelGGL(k_sp_hubs, rows, dim3(256), 0, st, L.rowptr, N, w.hubs, w.hub_cap, w.nhubs);
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }

  void mul(const double* Xs, double* W) {
    with_block_width(b, [&](auto B) { hipLaunchKernelGGL(k_sp_mul<decltype(B)::value>, mulgrid, dim3(256), 0, st, L, vb, Xs, W); });
    ++mults;
  }
  // W against q0 and the first na columns of V, twice; hcol >= 0: the coefficients are columns hcol .. of H
  void project(int na, int hcol) {
    for (int pass = 0; pass < 2; ++pass) {
      hipLaunchKernelGGL(k_sp_proj_part, red, dim3(256), 0, st, (const double*)V, ldv, na, (const double*)w.q0, (const double*)w.W, b, N, w.parts);
      hipLaunchKernelGGL(k_sp_proj_fin, one, dim3(256), 0, st, (const double*)w.parts, (na + 1) * b, w.C,
                         hcol >= 0 ? w.H + (size_t)ldh * (size_t)hcol : (double*)nullptr, ldh, na, b, w.nb, pass);
      with_block_width(b, [&](auto B) {
        hipLaunchKernelGGL(k_sp_axpy<decltype(B)::value>, rows, dim3(256), 0, st, (const double*)V, ldv, na, (const double*)w.q0, (const double*)w.C, w.W, N);
      });
    }
  }
  // W orthonormalised within itself, twice; its first width columns become columns col0 .. of V
  void orth(int col0, int width) {
    for (int pass = 0; pass < 2; ++pass) {
      gram_parts(w.W);
      hipLaunchKernelGGL(k_sp_chol, one, dim3(64), 0, st, (const double*)w.parts, b, width, pass == 0 ? 1 : 0, (const double*)w.nb, w.T,
                         pass == 1 ? w.flags + col0 : (int32_t*)nullptr);
      with_block_width(b, [&](auto B) {
        hipLaunchKernelGGL(k_sp_apply<decltype(B)::value>, rows, dim3(256), 0, st, w.W, (const double*)w.T, N, pass == 1 ? V : (double*)nullptr, ldv, col0,
                           width, w.Xs, (const double*)w.dis);
      });
    }
  }
  // the chunks of X' X (b x b) into parts; gram: added in order into G
  void gram_parts(const double* X) {
    hipLaunchKernelGGL(k_sp_proj_part, red, dim3(256), 0, st, X, b, b, (const double*)nullptr, X, b, N, w.parts);
  }
  void gram(const double* X) {
    gram_parts(X);
    hipLaunchKernelGGL(k_sp_proj_fin, one, dim3(256), 0, st, (const double*)w.parts, b * b, w.G, (double*)nullptr, 0, 0, b, (double*)nullptr, 0);
  }

  // the start block: projected, orthonormalised, the first columns of V
  int start(const double* d_start) {
    GFICF_HIP_CHECK(hipMemcpyAsync(w.W, d_start, sizeof(double) * (size_t)N * (size_t)b, hipMemcpyDeviceToDevice, st));
    project(0, -1);
    bw = b < mc ? b : mc;
    nc = bw;
    orth(0, bw);
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }

  // one cycle: the basis grown to mc columns (capped by m: to its last full block), then the remainder of the last block and its
  // Gram matrix.  From here to the restart nc is what the cycle ended with (me in spectral_ritz.h).
  int grow() {
    for (;;) {
      mul(w.Xs, w.W);
      project(nc, c0);
      if (nc == mc || (capped && mc - nc < b)) break;             // capped by m: no narrower block, no column of a remainder is discarded
      const int bwn = b < mc - nc ? b : mc - nc;
      orth(nc, bwn);
      c0 = nc; bw = bwn; nc += bwn;
    }
    gram(w.W);
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }

  // H, the Gram matrix, the column flags and the status word on the host: the cycle's one synchronisation
  int read_cycle() {
    uint32_t hst = 0;
    GFICF_HIP_CHECK(hipMemcpyAsync(hH.data(), w.H, sizeof(double) * (size_t)ldh * (size_t)nc, hipMemcpyDeviceToHost, st));
    GFICF_HIP_CHECK(hipMemcpyAsync(hG.data(), w.G, sizeof(double) * (size_t)b * b, hipMemcpyDeviceToHost, st));
    GFICF_HIP_CHECK(hipMemcpyAsync(hflags.data(), w.flags, sizeof(int32_t) * (size_t)nc, hipMemcpyDeviceToHost, st));
    GFICF_HIP_CHECK(hipMemcpyAsync(&hst, w.cc.status, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GFICF_HIP_CHECK(hipStreamSynchronize(st));
    if (hst & SP_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "a value of the graph that is not positive and finite");
    return GFICF_OK;
  }

  // Rayleigh-Ritz on the live columns; *can_restart: restarts are left and there is more in the cycle than a restart would keep
  int ritz(bool* can_restart) {
    const int n = sp_ritz(nc, keep, bw, b, ldh, rs.kept.data(), hH.data(), hflags.data(), hG.data(), tol, rz);
    if (n < b) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "the start block spans %d directions outside the trivial eigenvector, ndim = %d asked for", n, b);
    *can_restart = restarts < max_restarts && sp_keep_count(b, n) < nc;
    return GFICF_OK;
  }

  // X = V Z[:, :b], signed; the residuals recomputed from one more multiplication, converged decided on them.  Synchronises.
  int finish(double* d_X) {
    sp_final_rotation(rz, nc, b, zb);
    GFICF_HIP_CHECK(hipMemcpyAsync(w.Z, zb.data(), sizeof(double) * zb.size(), hipMemcpyHostToDevice, st));
    GFICF_HIP_CHECK(hipMemcpyAsync(w.theta, rz.theta.data(), sizeof(double) * (size_t)b, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sp_rotate, dim3(sp_grid(N * b)), dim3(256), 0, st, (const double*)V, ldv, nc, (const double*)w.Z, b, d_X, b, N);
    hipLaunchKernelGGL(k_sp_amax_part, red, dim3(64), 0, st, (const double*)d_X, b, N, w.pv, w.pi);
    hipLaunchKernelGGL(k_sp_sign_fin, one, dim3(64), 0, st, (const double*)d_X, b, (const double*)w.pv, (const int64_t*)w.pi, w.sign);
    hipLaunchKernelGGL(k_sp_flip_scale, dim3(sp_grid(N * b)), dim3(256), 0, st, d_X, b, N, (const double*)w.sign, (const double*)w.dis, w.Xfs);
    mul(w.Xfs, w.Wf);
    with_block_width(b, [&](auto B) {
      hipLaunchKernelGGL(k_sp_resid<decltype(B)::value>, rows, dim3(256), 0, st, w.Wf, (const double*)d_X, (const double*)w.theta, N);
    });
    gram(w.Wf);
    GFICF_HIP_CHECK(hipGetLastError());
    GFICF_HIP_CHECK(hipMemcpyAsync(hres.data(), w.G, sizeof(double) * (size_t)b * b, hipMemcpyDeviceToHost, st));
    GFICF_HIP_CHECK(hipStreamSynchronize(st));
    converged = 1;
    for (int l = 0; l < b; ++l) {
      resid[(size_t)l] = std::sqrt(hres[(size_t)l * b + l] > 0.0 ? hres[(size_t)l * b + l] : 0.0);
      if (!sp_within_tol(resid[(size_t)l], rz.theta[(size_t)l], tol)) converged = 0;
    }
    return GFICF_OK;
  }

  // thick restart: V <- V Z over the kept Ritz vectors, the residuals of the leading b (W_last Z_last) as the next block
  int restart() {
    ++restarts;
    sp_restart_choice(rz, nc, keep, bw, b, mc, rs);
    GFICF_HIP_CHECK(hipMemcpyAsync(w.Z, rs.up.data(), sizeof(double) * rs.up.size(), hipMemcpyHostToDevice, st));
    GFICF_HIP_CHECK(hipMemcpyAsync(w.Zl, rs.zl.data(), sizeof(double) * rs.zl.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sp_rotate, dim3(sp_grid(N * rs.kp)), dim3(256), 0, st, (const double*)V, ldv, nc, (const double*)w.Z, rs.kp, Vo, ldv, N);
    std::swap(V, Vo);
    with_block_width(b, [&](auto B) {
      hipLaunchKernelGGL(k_sp_apply<decltype(B)::value>, rows, dim3(256), 0, st, w.W, (const double*)w.Zl, N, (double*)nullptr, ldv, 0, 0, w.Xs,
                         (const double*)w.dis);
    });
    keep = rs.kp;
    project(keep, -1);
    bw = b < mc - keep ? b : mc - keep;
    orth(keep, bw);
    c0 = keep; nc = keep + bw;
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }
};

// the solve: theta, the residuals and the vectors on the device, h_info[1 .. 3] on the host.  Synchronises once per cycle, in every finish and at the end.
int sp_solve(gficf_ctx* ctx, const SpWs& w, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int b, const double* d_start,
             double tol, int m, int max_restarts, double* d_theta, double* d_resid, double* d_X, int64_t* h_info) {
  SpRun r(ctx, w, N, d_rowptr, d_col, d_val, b, tol, m, max_restarts);
  GFICF_RC(r.prepare());
  GFICF_RC(r.start(d_start));
  for (;;) {
    bool can_restart = false;
    GFICF_RC(r.grow());
    GFICF_RC(r.read_cycle());
    GFICF_RC(r.ritz(&can_restart));
    if (r.rz.pass || !can_restart) {
      GFICF_RC(r.finish(d_X));
      if (r.converged || !can_restart) break;
    }
    GFICF_RC(r.restart());
  }
  GFICF_HIP_CHECK(hipMemcpyAsync(d_theta, r.rz.theta.data(), sizeof(double) * (size_t)b, hipMemcpyHostToDevice, r.st));
  GFICF_HIP_CHECK(hipMemcpyAsync(d_resid, r.resid.data(), sizeof(double) * (size_t)b, hipMemcpyHostToDevice, r.st));
  GFICF_HIP_CHECK(hipStreamSynchronize(r.st));
  h_info[1] = r.restarts;
  h_info[2] = r.mults;
  h_info[3] = r.converged;
  return GFICF_OK;
}

}  // namespace

extern "C" {

int gficf_spectral_abi_version(void) { return GFICF_SPECTRAL_ABI_VERSION; }

size_t gficf_graph_components_workspace_bytes(int64_t N) {
  if (N < 1) return 0;
  CcWs w;
  return cc_carve(nullptr, w);
}

int gficf_graph_components_device(gficf_ctx* ctx, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, int64_t capacity, int32_t* d_labels,
                                  int64_t* d_info, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  if (N < 1 || N > 0x7FFFFFFFll) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld outside [1, 2^31)", (long long)N);
  if (capacity < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative capacity");
  if (!d_rowptr || !d_labels || !d_info || !ws || (capacity > 0 && !d_col)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  CcWs w;
  GFICF_RC(sp_take(ws, ws_bytes, [&](char* base) { return cc_carve(base, w); }));
  int64_t comps = 0, rounds = 0;
  return cc_run(ctx, w, N, d_rowptr, d_col, capacity, d_labels, d_info, &comps, &rounds);
}

size_t gficf_spectral_workspace_bytes(int64_t N, int64_t capacity, int ndim, int m) {
  if (N < 1 || capacity < 0 || ndim < 1 || ndim > GFICF_SPECTRAL_MAX_NDIM || m < 2 * ndim + 2 || m > GFICF_SPECTRAL_MAX_M) return 0;
  SpWs w;
  return sp_carve(nullptr, N, capacity, ndim, m, w);
}

int gficf_spectral_device(gficf_ctx* ctx, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t capacity, int ndim,
                          const double* d_start, double tol, int m, int max_restarts, void* ws, size_t ws_bytes, double* d_theta, double* d_resid,
                          double* d_vectors, int64_t* d_info) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(sp_check(N, capacity, ndim, tol, m, max_restarts));
  if (!d_rowptr || !d_start || !ws || !d_theta || !d_resid || !d_vectors || !d_info || (capacity > 0 && (!d_col || !d_val)))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  SpWs w;
  GFICF_RC(sp_take(ws, ws_bytes, [&](char* base) { return sp_carve(base, N, capacity, ndim, m, w); }));
  int64_t info[4] = {0, 0, 0, 0}, rounds = 0;
  GFICF_RC(cc_run(ctx, w.cc, N, d_rowptr, d_col, capacity, w.labels, w.ccinfo, &info[0], &rounds));
  if (info[0] == 1) GFICF_RC(sp_solve(ctx, w, N, d_rowptr, d_col, d_val, ndim, d_start, tol, m, max_restarts, d_theta, d_resid, d_vectors, info));
  GFICF_HIP_CHECK(hipMemcpyAsync(d_info, info, sizeof(info), hipMemcpyHostToDevice, ctx->stream));
  GFICF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return GFICF_OK;
}

int gficf_spectral_host(gficf_ctx* ctx, int64_t N, const int64_t* rowptr, const int32_t* col, const float* val, int ndim, const double* start,
                        double tol, int m, int max_restarts, int32_t* labels, double* theta, double* resid, double* vectors, int64_t* info) {
  GFICF_CTX_ENTER(ctx);
  if (!rowptr || !start || !theta || !resid || !vectors || !info) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  if (N < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld: no vertices", (long long)N);
  std::vector<int64_t> ptr;
  int64_t nnz = 0;
  GFICF_RC(gficf_host_colptr(rowptr, 1, N, "rowptr", ptr, &nnz));
  GFICF_RC(sp_check(N, nnz, ndim, tol, m, max_restarts));
  if (nnz > 0 && (!col || !val)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t ws_b = gficf_spectral_workspace_bytes(N, nnz, ndim, m), nb = (size_t)N * (size_t)ndim, e = (size_t)(nnz > 0 ? nnz : 1);
  gficf_host_io io{ctx, "gficf_spectral_host"};
  gficf_carver cv;
  int64_t *d_rowptr, *d_info; int32_t* d_col; float* d_val; double *d_start, *d_theta, *d_resid, *d_X; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_rowptr = cv.take<int64_t>((size_t)N + 1); d_col = cv.take<int32_t>(e); d_val = cv.take<float>(e); d_start = cv.take<double>(nb);
    d_theta = cv.take<double>(SP_MAXB); d_resid = cv.take<double>(SP_MAXB); d_X = cv.take<double>(nb); d_info = cv.take<int64_t>(4);
    d_ws = cv.take<char>(ws_b);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_rowptr, rowptr, sizeof(int64_t) * ((size_t)N + 1));
  io.up(d_col, col, sizeof(int32_t) * (size_t)nnz);
  io.up(d_val, val, sizeof(float) * (size_t)nnz);
  io.up(d_start, start, sizeof(double) * nb);
  if (!io.ok()) return io.drain(GFICF_OK);
  const int rc = gficf_spectral_device(ctx, N, d_rowptr, d_col, d_val, nnz, ndim, d_start, tol, m, max_restarts, d_ws, ws_b, d_theta, d_resid, d_X, d_info);
  if (rc) return io.drain(rc);
  io.down(info, d_info, sizeof(int64_t) * 4);
  if (labels) {                                                 // the labels of the entry's own components pass: the head of its workspace
    SpWs w;
    sp_carve(d_ws, N, nnz, ndim, m, w);
    io.down(labels, w.labels, sizeof(int32_t) * (size_t)N);
  }
  GFICF_RC(io.drain(GFICF_OK));
  if (info[0] == 1) {
    io.down(theta, d_theta, sizeof(double) * (size_t)ndim);
    io.down(resid, d_resid, sizeof(double) * (size_t)ndim);
    io.down(vectors, d_X, sizeof(double) * nb);
    return io.drain(GFICF_OK);
  }
  return GFICF_OK;
}

}  // extern "C"
