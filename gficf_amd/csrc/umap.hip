// umap.hip — runReduction: the UMAP / t-UMAP embedding of the cells (reference R/dimensinalityReduction.R:157-192 through
// uwot::tumap / uwot::umap).  Built into libgficf_umap.so, which links libgficf_hip.so and uses its context, pool, neighbour
// search, radix sort, scan and error plumbing (include/gficf_umap.h states the algorithm and what is relaxed).
//
// Launches of the graph stage (N points, k columns, M = 2 N k items: every membership once as (i, j) and once as (j, i)):
//   k_um_dist_part, k_um_dist_fin   the sum of all N k distances over UM_RED fixed chunks, the chunks added in order (f64);
//                                   non-finite distances flagged, negative ones taken as 0
//   k_um_smooth      one lane per point: rho, the bisection for sigma, the floor, the k memberships; bad ids flagged
//   (knn_symmetrise.h)   the items sorted by (row, column), a pair combined by um_combine, the kept entries emitted as CSR
// Launches of the layout stage:
//   k_addon_finite   the initial coordinates checked (addon_kernels.h)
//   k_um_wmax_part, k_um_wmax_fin, k_um_q   the largest value of P over fixed chunks; the 32-bit schedule word of every entry
//   k_um_hubs        the vertices whose row is longer than UM_HUB_LEN, listed (an integer counter: the list's order is free,
//                                   no result depends on it)
//   k_um_epoch       ONE per epoch.  A group of 8 lanes per vertex: the lanes fetch eight entries' columns, schedule words and
//                                   neighbour positions at once, the due ones are then applied in row order by every lane of
//                                   the group alike (operands handed round by shuffles), the negative samples of an entry
//                                   fetched by the lanes side by side before its attraction is computed.  The blocks behind
//                                   the vertex blocks walk the hub list with a whole wave per vertex, 64 entries per fetch.
// What bounds a sweep: the serial chain of the longest row (its due entries x (2 + negative_sample_rate) steps), since the
// running position passes through every step; everything else is latency hidden by the other groups.
#include <cmath>
#include <vector>

#include "addon_kernels.h"
#include "addon_status.h"
#include "common.h"
#include "gficf_umap.h"
#include "knn_symmetrise.h"
#include "umap_force.h"

namespace {

constexpr int UM_RED = 128;                  // fixed chunks of a reduction (one workgroup each)
constexpr int UM_HUB_LEN = 256;              // a row longer than this is walked by a whole wave
constexpr int UM_GROUP = 8;                  // lanes per vertex otherwise
constexpr int UM_HUB_WAVES = 1024;           // waves that share the hub list, at most
constexpr uint32_t UM_ST_ID = GFICF_AST_ID;          // a neighbour id outside [1, N], a column of P outside [0, N)
constexpr uint32_t UM_ST_VALUE = GFICF_AST_VALUE;    // a non-finite distance, a non-finite coordinate, a bad value of P
constexpr uint32_t UM_ST_CSC = GFICF_AST_CSC;        // a row pointer of P that decreases or leaves [0, capacity]

// one lane per element: n stays below 2^32 + 2 here (N k < 2^31), so the blocks fit a grid's x dimension
unsigned um_grid(int64_t n) { return (unsigned)gficf_ceil_div(n > 0 ? n : 1, 256); }

// ------------------------------------------------------------------------------------------------ graph: sigma, rho, W
__global__ __launch_bounds__(256) void k_um_dist_part(const float* __restrict__ dist, int64_t N, int k, int64_t ld, double* __restrict__ part,
                                                      uint32_t* __restrict__ status) {
  __shared__ double sh[256];
  const int64_t total = N * k, per = gficf_ceil_div(total, UM_RED);
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < total ? lo + per : total;
  double s = 0.0;
  bool bad = false;
  for (int64_t t = lo + threadIdx.x; t < hi; t += 256) {
    const float d = dist[(t / N) * ld + t % N];
    bad |= !isfinite(d);
    s += (double)uf_dist(d);
  }
  if (bad) atomicOr(status, UM_ST_VALUE);
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

__global__ void k_um_dist_fin(const double* __restrict__ part, int64_t total, float* __restrict__ mean) {
  double s = 0.0;
  for (int c = 0; c < UM_RED; ++c) s += part[c];
  *mean = (float)(s / (double)total);
}

__global__ __launch_bounds__(256) void k_um_smooth(const int32_t* __restrict__ idx, const float* __restrict__ dist, int64_t N, int k, int64_t ld,
                                                   int lc_floor, float lc_frac, const float* __restrict__ gmean, float* __restrict__ W,
                                                   float* __restrict__ sigma_out, float* __restrict__ rho_out, uint32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int cnt = 0;
  float nz_lo = 0.f, nz_hi = 0.f, nz_max = 0.f, rowsum = 0.f;
  for (int c = 0; c < k; ++c) {
    const float d = uf_dist(dist[(int64_t)c * ld + i]);
    rowsum += d;
    if (c >= 1 && d > 0.f) {
      ++cnt;
      if (cnt == lc_floor) nz_lo = d;
      if (cnt == lc_floor + 1) nz_hi = d;
      nz_max = fmaxf(nz_max, d);
    }
  }
  float rho = 0.f;
  if (cnt >= lc_floor) {
    rho = nz_lo;
    if (lc_frac > 0.f && cnt > lc_floor) rho = nz_lo + lc_frac * (nz_hi - nz_lo);
  } else if (cnt > 0) {
    rho = nz_max;
  }
  const float target = log2f((float)k);
  float lo = 0.f, hi = INFINITY, mid = 1.f;
  for (int it = 0; it < 64; ++it) {
    float psum = 0.f;
    for (int c = 1; c < k; ++c) {
      const float x = uf_dist(dist[(int64_t)c * ld + i]) - rho;
      psum += x > 0.f ? expf(-x / mid) : 1.f;
    }
    if (fabsf(psum - target) < 1e-5f) break;
    if (psum > target) {
      hi = mid;
      mid = (lo + hi) * 0.5f;
    } else {
      lo = mid;
      mid = isinf(hi) ? mid * 2.f : (lo + hi) * 0.5f;
    }
  }
  const float floor_v = 1e-3f * (rho > 0.f ? rowsum / (float)k : *gmean);
  const float sigma = fmaxf(mid, floor_v);
  if (sigma_out) sigma_out[i] = sigma;
  if (rho_out) rho_out[i] = rho;
  bool bad = false;
  for (int c = 0; c < k; ++c) {
    const int32_t j = idx[(int64_t)c * ld + i];
    const float x = uf_dist(dist[(int64_t)c * ld + i]) - rho;
    float w;
    if (j < 1 || (int64_t)j > N) {
      bad = true;
      w = 0.f;
    } else if ((int64_t)j - 1 == i) {
      w = 0.f;
    } else if (x <= 0.f || sigma == 0.f) {
      w = 1.f;
    } else {
      w = expf(-x / sigma);
    }
    W[(int64_t)c * N + i] = w > 0.f ? w : 0.f;                  // (a NaN distance, flagged above, leaves no entry)
  }
  if (bad) atomicOr(status, UM_ST_ID);
}

// ------------------------------------------------------------------------------------------------ graph: symmetrisation
// the two memberships of a pair, smaller first: both directions evaluate the same expression on the same operands
struct um_combine {
  float mix;
  __device__ float operator()(float x, float y) const {
    const float lo = fminf(x, y), hi = fmaxf(x, y), prod = lo * hi;
    return mix * ((lo + hi) - prod) + (1.f - mix) * prod;
  }
};

// ------------------------------------------------------------------------------------------------ layout: schedule
__global__ __launch_bounds__(256) void k_um_wmax_part(const float* __restrict__ val, const int64_t* __restrict__ rowptr, int64_t N, int64_t cap,
                                                      float* __restrict__ part, uint32_t* __restrict__ status) {
  __shared__ float sh[256];
  const int64_t total = gficf_addon_nnz(rowptr, N, cap), per = gficf_ceil_div(total, UM_RED);
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < total ? lo + per : total;
  float m = 0.f;
  bool bad = false;
  for (int64_t t = lo + threadIdx.x; t < hi; t += 256) {
    const float w = val[t];
    if (w > 0.f && !isinf(w)) m = fmaxf(m, w);
    else bad = true;
  }
  if (bad) atomicOr(status, UM_ST_VALUE);
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] = fmaxf(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

__global__ void k_um_wmax_fin(const float* __restrict__ part, float* __restrict__ wmax, uint32_t* __restrict__ nhubs) {
  float m = 0.f;
  for (int c = 0; c < UM_RED; ++c) m = fmaxf(m, part[c]);
  *wmax = m;
  *nhubs = 0u;
}

__global__ __launch_bounds__(256) void k_um_q(const float* __restrict__ val, const int32_t* __restrict__ col, const int64_t* __restrict__ rowptr,
                                              int64_t N, int64_t cap, const float* __restrict__ wmax, uint32_t* __restrict__ q,
                                              uint32_t* __restrict__ status) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= cap) return;
  uint32_t qe = 0u;
  if (e < gficf_addon_nnz(rowptr, N, cap)) {
    const float w = val[e];
    const int32_t j = col[e];
    if (j < 0 || (int64_t)j >= N) atomicOr(status, UM_ST_ID);
    else if (w > 0.f && !isinf(w)) {
      const double x = floor((double)w / (double)*wmax * 4294967296.0);
      qe = x >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)x;
    }
  }
  q[e] = qe;
}

__global__ __launch_bounds__(256) void k_um_hubs(const int64_t* __restrict__ rowptr, int64_t N, int64_t cap, int32_t* __restrict__ hubs,
                                                 uint32_t hub_cap, uint32_t* __restrict__ nhubs, uint32_t* __restrict__ status) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= N) return;
  const int64_t b = rowptr[v], e = rowptr[v + 1];
  if (b < 0 || e < b || e > cap || (v == 0 && b != 0)) {
    atomicOr(status, UM_ST_CSC);
    return;
  }
  if (e - b > UM_HUB_LEN) {
    const uint32_t at = atomicAdd(nhubs, 1u);
    if (at < hub_cap) hubs[at] = (int32_t)v;
  }
}

// ------------------------------------------------------------------------------------------------ layout: one epoch
struct UmLay {
  int64_t N, cap;
  const int64_t* rowptr;
  const int32_t* col;
  const uint32_t* q;
  const int32_t* hubs;
  const uint32_t* nhubs;
  uint32_t hub_cap;
  float a, b, m2ab, g2b;          // -2ab, 2 gamma b
  int rate;
  u64 seed;
};

// vertex v by the G lanes lane0 .. lane0 + G - 1 of a wave (all of them here, with the same v)
template <int G, bool T1>
__device__ inline void um_vertex(const UmLay& L, int32_t v, const float2* __restrict__ Ycur, float2* __restrict__ Ynext, int n, float alpha) {
  const int wl = threadIdx.x & 63, lane = wl & (G - 1), lane0 = wl - lane;
  int64_t e0 = L.rowptr[v], e1 = L.rowptr[v + 1];
  if (e0 < 0) e0 = 0;
  if (e1 > L.cap) e1 = L.cap;
  const float2 y0 = Ycur[v];
  float yx = y0.x, yy = y0.y;
  const u64 kn = uf_mix(L.seed + (u64)n), un = (u64)n;
  for (int64_t base = e0; base < e1; base += G) {
    const int64_t e = base + lane;
    bool due = false;
    float2 yj = make_float2(0.f, 0.f);
    if (e < e1) {
      const u64 qe = (u64)L.q[e];
      const int32_t j = L.col[e];
      due = (((un + 1ull) * qe) >> 32) > ((un * qe) >> 32) && j >= 0 && (int64_t)j < L.N;
      if (due) yj = Ycur[j];
    }
    u64 mask = __ballot(due) >> lane0;
    if (G < 64) mask &= (1ull << G) - 1ull;
    while (mask) {                                              // the same in every lane of the group
      const int t = __builtin_ctzll(mask);
      mask &= mask - 1ull;
      const u64 ke = uf_mix(kn + (u64)(base + t));
      for (int s0 = 0;; s0 += G) {                              // the first round also applies the attraction
        int32_t jn = v;                                         // v: no sample
        float2 yn = make_float2(0.f, 0.f);
        if (s0 + lane < L.rate) {
          const u64 key = uf_mix(ke + (u64)(s0 + lane));
          jn = (int32_t)(((key >> 32) * (u64)L.N) >> 32);
          if (jn != v) yn = Ycur[jn];
        }
        if (s0 == 0) {
          const float jx = __shfl(yj.x, t, G), jy = __shfl(yj.y, t, G);
          uf_attract<T1>(yx, yy, jx, jy, alpha, L);
          uf_attract<T1>(yx, yy, jx, jy, alpha, L);
        }
        const int cnt = L.rate - s0 < G ? L.rate - s0 : G;
        for (int u = 0; u < cnt; ++u) {
          const int32_t ju = __shfl(jn, u, G);
          const float nx = __shfl(yn.x, u, G), ny = __shfl(yn.y, u, G);
          if (ju != v) uf_repulse<T1>(yx, yy, nx, ny, alpha, L);
        }
        if (s0 + G >= L.rate) break;
      }
    }
  }
  if (lane == 0) Ynext[v] = make_float2(yx, yy);
}

template <bool T1>
__global__ __launch_bounds__(256) void k_um_epoch(UmLay L, unsigned vertex_blocks, const float2* __restrict__ Ycur, float2* __restrict__ Ynext, int n,
                                                  float alpha) {
  if (blockIdx.x < vertex_blocks) {
    const int64_t v = (int64_t)blockIdx.x * (256 / UM_GROUP) + threadIdx.x / UM_GROUP;
    if (v >= L.N) return;
    const int64_t len = L.rowptr[v + 1] - L.rowptr[v];
    if (len > UM_HUB_LEN) return;                               // a wave of the blocks behind takes it
    um_vertex<UM_GROUP, T1>(L, (int32_t)v, Ycur, Ynext, n, alpha);
  } else {
    const uint32_t waves = (gridDim.x - vertex_blocks) * 4u, wave = (blockIdx.x - vertex_blocks) * 4u + threadIdx.x / 64u;
    uint32_t nh = *L.nhubs;
    if (nh > L.hub_cap) nh = L.hub_cap;
    for (uint32_t h = wave; h < nh; h += waves) um_vertex<64, T1>(L, L.hubs[h], Ycur, Ynext, n, alpha);
  }
}

// ------------------------------------------------------------------------------------------------ boundary conversions (chain)
__global__ __launch_bounds__(256) void k_um_in(const double* __restrict__ init, int64_t N, float* __restrict__ Y, uint32_t* __restrict__ status) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * N) return;
  const double x = init[(t & 1) * N + (t >> 1)];
  if (!isfinite(x)) atomicOr(status, UM_ST_VALUE);
  Y[t] = (float)x;
}

// ------------------------------------------------------------------------------------------------ workspaces
struct UmGraphWs {
  uint32_t* status;
  double* part;
  float* mean;
  float* W;
  SymWs sym;
};

size_t um_carve_graph(char* base, int64_t N, int k, UmGraphWs& w) {
  gficf_carver cv;
  cv.base = base;
  w.status = cv.take<uint32_t>(1);
  w.part = cv.take<double>(UM_RED);
  w.mean = cv.take<float>(1);
  w.W = cv.take<float>((size_t)N * (size_t)k);
  sym_carve(cv, N, 2 * (size_t)N * (size_t)k, w.sym);
  return cv.total();
}

struct UmLayoutWs {
  uint32_t* status;
  uint32_t* q;
  float* Y1;
  float* part;
  float* wmax;
  uint32_t* nhubs;
  int32_t* hubs;
  uint32_t hub_cap;
};

size_t um_carve_layout(char* base, int64_t N, int64_t cap, UmLayoutWs& w) {
  gficf_carver cv;
  cv.base = base;
  w.hub_cap = (uint32_t)(cap / UM_HUB_LEN + 1);
  w.status = cv.take<uint32_t>(1);
  w.q = cv.take<uint32_t>((size_t)(cap > 0 ? cap : 1));
  w.Y1 = cv.take<float>(2 * (size_t)N);
  w.part = cv.take<float>(UM_RED);
  w.wmax = cv.take<float>(1);
  w.nhubs = cv.take<uint32_t>(1);
  w.hubs = cv.take<int32_t>(w.hub_cap);
  return cv.total();
}

int um_check_graph(int64_t N, int k, int64_t ld, double lc, double mix) {
  if (N < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld: no points", (long long)N);
  if (k < 2 || k > GFICF_KNN_MAX_K) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_neighbors = %d outside [2, %d]", k, GFICF_KNN_MAX_K);
  if ((int64_t)k > N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_neighbors = %d exceeds N = %lld points", k, (long long)N);
  if (N * k >= ((int64_t)1 << 31)) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "N * n_neighbors = %lld reaches 2^31", (long long)(N * k));
  if (ld < N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ld = %lld < N = %lld", (long long)ld, (long long)N);
  if (!(lc >= 1.0) || !(lc <= (double)GFICF_KNN_MAX_K)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "local_connectivity = %g outside [1, %d]", lc, GFICF_KNN_MAX_K);
  if (!(mix >= 0.0 && mix <= 1.0)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "set_op_mix_ratio = %g outside [0, 1]", mix);
  return GFICF_OK;
}

int um_check_layout(int64_t N, int64_t cap, double a, double b, double gamma, double lr, int rate, int n_epochs, int eb, int ee) {
  if (N < 1 || N > 0x7FFFFFFFll) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld outside [1, 2^31)", (long long)N);
  if (cap < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative capacity");
  if (!(a > 0.0) || !(b > 0.0) || !std::isfinite(a) || !std::isfinite(b)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a = %g, b = %g must be positive", a, b);
  if (!std::isfinite(gamma) || !std::isfinite(lr)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "repulsion_strength / learning_rate not finite");
  if (rate < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative_sample_rate = %d", rate);
  if (n_epochs < 1 || eb < 0 || ee < eb || ee > n_epochs)
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "epochs [%d, %d) of %d", eb, ee, n_epochs);
  return GFICF_OK;
}

// the graph stage on a carved workspace whose status word the caller has zeroed
int um_graph(gficf_ctx* ctx, const UmGraphWs& w, const int32_t* d_idx, const float* d_dist, int64_t N, int k, int64_t ld, double lc, double mix,
             int64_t* d_rowptr, int32_t* d_col, float* d_val, int64_t* d_nnz, float* d_sigma, float* d_rho) {
  hipStream_t st = ctx->stream;
  const int lcf = (int)std::floor(lc);
  hipLaunchKernelGGL(k_um_dist_part, dim3(UM_RED), dim3(256), 0, st, d_dist, N, k, ld, w.part, w.status);
  hipLaunchKernelGGL(k_um_dist_fin, dim3(1), dim3(1), 0, st, (const double*)w.part, N * k, w.mean);
  hipLaunchKernelGGL(k_um_smooth, dim3(um_grid(N)), dim3(256), 0, st, d_idx, d_dist, N, k, ld, lcf, (float)(lc - (double)lcf), (const float*)w.mean,
                     w.W, d_sigma, d_rho, w.status);
  return sym_enqueue(ctx, w.sym, d_idx, 0, w.W, N, k, ld, um_combine{(float)mix}, d_rowptr, d_col, d_val, d_nnz);
}

// the layout stage, likewise
int um_layout(gficf_ctx* ctx, const UmLayoutWs& w, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t cap, float a,
              float b, float gamma, float lr, int rate, int n_epochs, int eb, int ee, uint64_t seed, float* d_Y) {
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_addon_finite, dim3(um_grid(2 * N) < 1024 ? um_grid(2 * N) : 1024), dim3(256), 0, st, (const float*)d_Y, 2 * N, w.status);
  hipLaunchKernelGGL(k_um_wmax_part, dim3(UM_RED), dim3(256), 0, st, d_val, d_rowptr, N, cap, w.part, w.status);
  hipLaunchKernelGGL(k_um_wmax_fin, dim3(1), dim3(1), 0, st, (const float*)w.part, w.wmax, w.nhubs);
  if (cap > 0)
    hipLaunchKernelGGL(k_um_q, dim3((unsigned)gficf_ceil_div(cap, 256)), dim3(256), 0, st, d_val, d_col, d_rowptr, N, cap, (const float*)w.wmax, w.q,
                       w.status);
  hipLaunchKernelGGL(k_um_hubs, dim3((unsigned)gficf_ceil_div(N, 256)), dim3(256), 0, st, d_rowptr, N, cap, w.hubs, w.hub_cap, w.nhubs, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  UmLay L;
  L.N = N; L.cap = cap; L.rowptr = d_rowptr; L.col = d_col; L.q = w.q; L.hubs = w.hubs; L.nhubs = w.nhubs; L.hub_cap = w.hub_cap;
  L.a = a; L.b = b; L.m2ab = -2.f * a * b; L.g2b = 2.f * gamma * b; L.rate = rate; L.seed = (u64)seed;
  const bool t1 = a == 1.f && b == 1.f;
  const unsigned vb = (unsigned)gficf_ceil_div(N, 256 / UM_GROUP);
  const int64_t hw = w.hub_cap < (uint32_t)UM_HUB_WAVES ? (int64_t)w.hub_cap : (int64_t)UM_HUB_WAVES;
  const unsigned hb = (unsigned)gficf_ceil_div(hw, 4);
  float *cur = d_Y, *nxt = w.Y1;
  for (int n = eb; n < ee; ++n) {
    const float alpha = lr * (1.f - (float)n / (float)n_epochs);
    if (t1)
      hipLaunchKernelGGL(k_um_epoch<true>, dim3(vb + hb), dim3(256), 0, st, L, vb, (const float2*)cur, (float2*)nxt, n, alpha);
    else
      hipLaunchKernelGGL(k_um_epoch<false>, dim3(vb + hb), dim3(256), 0, st, L, vb, (const float2*)cur, (float2*)nxt, n, alpha);
    float* t = cur; cur = nxt; nxt = t;
  }
  GFICF_HIP_CHECK(hipGetLastError());
  if (cur != d_Y) GFICF_HIP_CHECK(hipMemcpyAsync(d_Y, cur, sizeof(float) * 2 * (size_t)N, hipMemcpyDeviceToDevice, st));
  return GFICF_OK;
}

}  // namespace

extern "C" {

int gficf_umap_abi_version(void) { return GFICF_UMAP_ABI_VERSION; }

size_t gficf_umap_graph_workspace_bytes(int64_t N, int k) {
  if (N < 1 || k < 2 || k > GFICF_KNN_MAX_K || N * k >= ((int64_t)1 << 31)) return 0;
  UmGraphWs w;
  return um_carve_graph(nullptr, N, k, w);
}

int gficf_umap_graph_device(gficf_ctx* ctx, const int32_t* d_idx, const float* d_dist, int64_t N, int k, int64_t ld, double local_connectivity,
                            double set_op_mix_ratio, void* ws, size_t ws_bytes, int64_t* d_rowptr, int32_t* d_col, float* d_val, int64_t capacity,
                            int64_t* d_nnz, float* d_sigma, float* d_rho, float* d_w) {
  GFICF_CTX_ENTER(ctx);
  const int rc = um_check_graph(N, k, ld, local_connectivity, set_op_mix_ratio);
  if (rc) return rc;
  if (!d_idx || !d_dist || !ws || !d_rowptr || !d_col || !d_val || !d_nnz) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (capacity < 2 * N * k) GFICF_FAIL(GFICF_ERR_CAPACITY, "capacity %lld < 2 N k = %lld entries", (long long)capacity, (long long)(2 * N * k));
  UmGraphWs w;
  const size_t need = um_carve_graph(nullptr, N, k, w);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  um_carve_graph((char*)ws, N, k, w);
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), ctx->stream));
  const int rg = um_graph(ctx, w, d_idx, d_dist, N, k, ld, local_connectivity, set_op_mix_ratio, d_rowptr, d_col, d_val, d_nnz, d_sigma, d_rho);
  if (rg) return rg;
  if (d_w) GFICF_HIP_CHECK(hipMemcpyAsync(d_w, w.W, sizeof(float) * (size_t)N * (size_t)k, hipMemcpyDeviceToDevice, ctx->stream));
  return GFICF_OK;
}

size_t gficf_umap_layout_workspace_bytes(int64_t N, int64_t capacity) {
  if (N < 1 || capacity < 0) return 0;
  UmLayoutWs w;
  return um_carve_layout(nullptr, N, capacity, w);
}

int gficf_umap_layout_device(gficf_ctx* ctx, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t capacity, float a,
                             float b, float gamma, float learning_rate, int negative_sample_rate, int n_epochs, int epoch_begin, int epoch_end,
                             uint64_t seed, float* d_Y, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  const int rc = um_check_layout(N, capacity, a, b, gamma, learning_rate, negative_sample_rate, n_epochs, epoch_begin, epoch_end);
  if (rc) return rc;
  if (!d_rowptr || !d_Y || !ws || (capacity > 0 && (!d_col || !d_val))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  UmLayoutWs w;
  const size_t need = um_carve_layout(nullptr, N, capacity, w);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  um_carve_layout((char*)ws, N, capacity, w);
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), ctx->stream));
  return um_layout(ctx, w, N, d_rowptr, d_col, d_val, capacity, a, b, gamma, learning_rate, negative_sample_rate, n_epochs, epoch_begin, epoch_end,
                   seed, d_Y);
}

int gficf_umap_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  const int rc = gficf_addon_read_status(ctx, ws, &st);
  if (rc) return rc;
  if (st & UM_ST_ID) GFICF_FAIL(GFICF_ERR_BAD_ID, "a neighbour id outside [1, N] or a column of the graph outside [0, N)");
  if (st & UM_ST_CSC) GFICF_FAIL(GFICF_ERR_BAD_CSC, "a row pointer of the graph decreases or leaves [0, capacity]");
  if (st & UM_ST_VALUE)
    GFICF_FAIL(GFICF_ERR_BAD_VALUE, "a non-finite distance, a non-finite initial coordinate or a value of the graph that is not positive");
  return GFICF_OK;
}

int gficf_umap_host(gficf_ctx* ctx, const double* X, int64_t N, int d, int64_t ld, int metric, int n_neighbors, double local_connectivity,
                    double set_op_mix_ratio, double a, double b, double gamma, double learning_rate, int negative_sample_rate, int n_epochs,
                    const double* init, uint64_t seed, double* embedding, int64_t* rowptr, int32_t* col, float* val, int64_t* nnz, int32_t* idx,
                    float* dist) {
  GFICF_CTX_ENTER(ctx);
  const int k = n_neighbors;
  int rc = um_check_graph(N, k, ld, local_connectivity, set_op_mix_ratio);
  if (rc) return rc;
  const int64_t cap = 2 * N * k;
  rc = um_check_layout(N, cap, a, b, gamma, learning_rate, negative_sample_rate, n_epochs, 0, n_epochs);
  if (rc) return rc;
  if (d < 1 || gficf_knn_dpad(d) < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "d = %d outside [1, 128]", d);
  if (!gficf_knn_metric_ok(metric)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "unknown metric %d", metric);
  if (!X || !init || !embedding) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const bool want_graph = rowptr || col || val || nnz;
  if (want_graph && (!rowptr || !col || !val || !nnz)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "the graph is returned whole: rowptr, col, val and nnz");
  const size_t nk = (size_t)N * (size_t)k, dpad = (size_t)gficf_knn_dpad(d);
  const size_t knn_b = gficf_knn_workspace_bytes(ctx, N, N, k), gr_b = gficf_umap_graph_workspace_bytes(N, k),
               ly_b = gficf_umap_layout_workspace_bytes(N, cap);
  UmGraphWs gw;
  UmLayoutWs lw;
  gficf_host_io io{ctx, "gficf_umap_host"};
  gficf_carver cv;
  double *d_X, *d_init, *d_emb; float *d_pts, *d_dist, *d_val, *d_Y; int32_t *d_idx, *d_col; int64_t *d_rowptr, *d_nnz; char *d_kws, *d_gws, *d_lws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_lws = cv.take<char>(ly_b);                                // first: its head is the status word of the whole chain
    d_X = cv.take<double>((size_t)ld * (size_t)d); d_init = cv.take<double>(2 * (size_t)N); d_emb = cv.take<double>(2 * (size_t)N);
    d_pts = cv.take<float>((size_t)N * dpad); d_idx = cv.take<int32_t>(nk); d_dist = cv.take<float>(nk);
    d_rowptr = cv.take<int64_t>((size_t)N + 1); d_col = cv.take<int32_t>((size_t)cap); d_val = cv.take<float>((size_t)cap);
    d_nnz = cv.take<int64_t>(1); d_Y = cv.take<float>(2 * (size_t)N);
    d_kws = cv.take<char>(knn_b); d_gws = cv.take<char>(gr_b);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_X, X, sizeof(double) * (size_t)ld * (size_t)d);
  io.up(d_init, init, sizeof(double) * 2 * (size_t)N);
  int64_t h_nnz = 0;
  if (io.ok()) {
    hipStream_t st = ctx->stream;
    um_carve_graph(d_gws, N, k, gw);
    um_carve_layout(d_lws, N, cap, lw);
    gw.status = lw.status;                                      // one status word: what gficf_umap_sync(ctx, d_lws) reads
    io.e = hipMemsetAsync(lw.status, 0, sizeof(uint32_t), st);
    if (io.ok()) {
      rc = gficf_knn_prepare_device(ctx, d_X, 1, N, d, ld, metric, d_pts);
      if (!rc) rc = gficf_knn_search_device(ctx, d_pts, N, d, k, metric, 0, N, d_kws, knn_b, d_idx, d_dist, N);
      if (!rc) rc = um_graph(ctx, gw, d_idx, d_dist, N, k, N, local_connectivity, set_op_mix_ratio, d_rowptr, d_col, d_val, d_nnz, nullptr, nullptr);
      if (!rc) {
        hipLaunchKernelGGL(k_um_in, dim3(um_grid(2 * N)), dim3(256), 0, st, (const double*)d_init, N, d_Y, lw.status);
        rc = um_layout(ctx, lw, N, d_rowptr, d_col, d_val, cap, (float)a, (float)b, (float)gamma, (float)learning_rate, negative_sample_rate,
                       n_epochs, 0, n_epochs, seed, d_Y);
      }
      if (!rc) {
        hipLaunchKernelGGL(k_addon_out, dim3(um_grid(2 * N)), dim3(256), 0, st, (const float*)d_Y, N, d_emb);
        io.e = hipGetLastError();
        io.down(embedding, d_emb, sizeof(double) * 2 * (size_t)N);
        if (idx) io.down(idx, d_idx, sizeof(int32_t) * nk);
        if (dist) io.down(dist, d_dist, sizeof(float) * nk);
        if (want_graph) {
          io.down(rowptr, d_rowptr, sizeof(int64_t) * ((size_t)N + 1));
          io.down(&h_nnz, d_nnz, sizeof(int64_t));
        }
      }
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  rc = gficf_umap_sync(ctx, d_lws);
  if (rc) return rc;
  if (want_graph) {                                             // the entries in use only (their count has just arrived)
    *nnz = h_nnz;
    io.down(col, d_col, sizeof(int32_t) * (size_t)h_nnz);
    io.down(val, d_val, sizeof(float) * (size_t)h_nnz);
    return io.finish(GFICF_OK);
  }
  return GFICF_OK;
}

}  // extern "C"
