// transform.hip — embedNewCells / classify.cells (reference R/cellClassifier.R:15-95 through uwot::umap_transform and class::knn):
// new cells placed into a trained UMAP / t-UMAP plane and labelled by their trained neighbours.  Built into
// libgficf_transform.so, which links libgficf_hip.so and uses its context, pool, gficf_knn_prepare_device and error plumbing
// (include/gficf_transform.h states the algorithm and what is relaxed).
//
// Launches (N trained cells, M new cells, k neighbours):
//   search    k_knn_tiles<.., plain> (knn_tiles.h: the square search's own tile kernel, one text), k_tr_merge (transform_search.h)
//                              the M x k table over all N training rows
//   weights   k_tr_smooth      one lane per new cell: rho, the bisection for sigma, the row-local floor, the k memberships; bad ids
//                              and non-finite distances flagged
//   init      k_addon_finite, k_tr_init   the trained plane checked; one lane per new cell: the weighted mean of its k heads
//   layout    k_addon_finite, k_tr_layout   ONE launch for the whole epoch range.  A group of 8 lanes per new cell.  The trained
//                              cells do not move, so the group reads its row once: the k schedule words and the k head
//                              positions go to LDS and stay there for every epoch; the running position stays in registers;
//                              per due entry the lanes fetch the negative samples side by side before the attraction is
//                              computed, and every lane of the group applies the steps alike (operands handed round by
//                              shuffles).  Y is written once, at the end.
//   vote      k_tr_vote        one lane per new cell, its row's labels in LDS
// What bounds the layout: the serial chain of one cell — (epochs) x (due entries) x (1 + negative_sample_rate) dependent steps
// with one round of gathers per due entry; the cells are independent, so everything else is latency hidden by other groups.
#include <cmath>
#include <vector>

#include "addon_kernels.h"
#include "addon_status.h"
#include "common.h"
#include "gficf_transform.h"
#include "transform_search.h"
#include "umap_force.h"

namespace {

constexpr int TR_GROUP = 8;                  // lanes per new cell in the layout
constexpr int TR_LAY_THREADS = 64;           // one wave = 8 cells per workgroup: few cells still spread over many CUs
constexpr int TR_VOTE_THREADS = 64;
constexpr uint32_t TR_ST_ID = GFICF_AST_ID;          // a neighbour id outside [1, N], a label outside [0, C)
constexpr uint32_t TR_ST_VALUE = GFICF_AST_VALUE;    // a non-finite distance, membership or coordinate

unsigned tr_grid(int64_t n, int per = 256) { return (unsigned)gficf_ceil_div(n > 0 ? n : 1, per); }

// ------------------------------------------------------------------------------------------------ memberships
__global__ __launch_bounds__(256) void k_tr_smooth(const int32_t* __restrict__ idx, const float* __restrict__ dist, int64_t N, int64_t M, int k,
                                                   int64_t ld, int lc_floor, float lc_frac, float* __restrict__ W, int64_t ld_w,
                                                   float* __restrict__ sigma_out, float* __restrict__ rho_out, uint32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  int cnt = 0;
  float nz_first = 0.f, nz_lo = 0.f, nz_hi = 0.f, nz_max = 0.f, rowsum = 0.f;
  bool bad_v = false;
  for (int c = 0; c < k; ++c) {
    const float raw = dist[(int64_t)c * ld + i];
    bad_v |= !isfinite(raw);
    const float d = uf_dist(raw);
    rowsum += d;
    if (d > 0.f) {
      ++cnt;
      if (cnt == 1) nz_first = d;
      if (cnt == lc_floor) nz_lo = d;
      if (cnt == lc_floor + 1) nz_hi = d;
      nz_max = fmaxf(nz_max, d);
    }
  }
  float rho = 0.f;
  if (lc_floor == 0) {
    rho = cnt > 0 ? lc_frac * nz_first : 0.f;
  } else if (cnt >= lc_floor) {
    rho = nz_lo;
    if (lc_frac > 0.f && cnt > lc_floor) rho = nz_lo + lc_frac * (nz_hi - nz_lo);
  } else if (cnt > 0) {
    rho = nz_max;
  }
  const float target = log2f((float)k);
  float lo = 0.f, hi = INFINITY, mid = 1.f;
  for (int it = 0; it < 64; ++it) {
    float psum = 0.f;
    for (int c = 0; c < k; ++c) {
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
  const float sigma = fmaxf(mid, 1e-3f * (rowsum / (float)k));      // the row's own mean, whatever rho is
  if (sigma_out) sigma_out[i] = sigma;
  if (rho_out) rho_out[i] = rho;
  bool bad_id = false;
  for (int c = 0; c < k; ++c) {
    const int32_t j = idx[(int64_t)c * ld + i];
    const float x = uf_dist(dist[(int64_t)c * ld + i]) - rho;
    float w;
    if (j < 1 || (int64_t)j > N) {
      bad_id = true;
      w = 0.f;
    } else if (x <= 0.f || sigma == 0.f) {
      w = 1.f;
    } else {
      w = expf(-x / sigma);
    }
    W[(int64_t)c * ld_w + i] = w > 0.f ? w : 0.f;                   // (a NaN distance, flagged above, leaves no membership)
  }
  if (bad_id) atomicOr(status, TR_ST_ID);
  if (bad_v) atomicOr(status, TR_ST_VALUE);
}

// ------------------------------------------------------------------------------------------------ initial position
__global__ __launch_bounds__(256) void k_tr_init(const int32_t* __restrict__ idx, int64_t ld, const float* __restrict__ W, int64_t ld_w,
                                                 const float2* __restrict__ Yt, int64_t N, int64_t M, int k, float2* __restrict__ Y,
                                                 uint32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  float sw = 0.f, sx = 0.f, sy = 0.f, mx = 0.f, my = 0.f;
  bool bad_id = false, bad_v = false;
  for (int c = 0; c < k; ++c) {
    const int32_t j = idx[(int64_t)c * ld + i];
    const float w = W[(int64_t)c * ld_w + i];
    if (j < 1 || (int64_t)j > N) { bad_id = true; continue; }
    if (!(w >= 0.f) || isinf(w)) { bad_v = true; continue; }
    const float2 yj = Yt[j - 1];
    sw = sw + w;
    sx = sx + w * yj.x;
    sy = sy + w * yj.y;
    mx = mx + yj.x;
    my = my + yj.y;
  }
  Y[i] = sw > 0.f ? make_float2(sx / sw, sy / sw) : make_float2(mx / (float)k, my / (float)k);
  if (bad_id) atomicOr(status, TR_ST_ID);
  if (bad_v) atomicOr(status, TR_ST_VALUE);
}

// ------------------------------------------------------------------------------------------------ layout: every epoch, one launch
struct TrLay {
  const int32_t* idx;
  int64_t ld;
  const float* W;
  int64_t ld_w;
  const float2* Yt;
  int64_t N, M;
  int k;
  float a, b, m2ab, g2b, lr;      // -2ab, 2 gamma b
  int rate, n_epochs, eb, ee;
  u64 seed, qoff;
  float2* Y;
  uint32_t* status;
};

// LDS per workgroup: [8 cells][k] head positions (float2), then [8 cells][k] schedule words
size_t tr_layout_lds(int k) { return (size_t)(TR_LAY_THREADS / TR_GROUP) * (size_t)k * (sizeof(float2) + sizeof(uint32_t)); }

template <bool T1>
__global__ __launch_bounds__(TR_LAY_THREADS) void k_tr_layout(const TrLay L) {
  constexpr int G = TR_GROUP, CELLS = TR_LAY_THREADS / TR_GROUP;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int k = L.k;
  const int lane = threadIdx.x & (G - 1), g = threadIdx.x / G, lane0 = threadIdx.x - lane;     // the workgroup is one wave
  float2* const sY = reinterpret_cast<float2*>(smem) + (size_t)g * k;
  uint32_t* const sQ = reinterpret_cast<uint32_t*>(reinterpret_cast<float2*>(smem) + (size_t)CELLS * k) + (size_t)g * k;
  const int64_t i = (int64_t)blockIdx.x * CELLS + g;
  if (i >= L.M) return;                                           // whole groups leave: the others' ballots and shuffles stay inside a group

  // the row, once: the largest membership, then schedule word and head position of every entry
  bool bad_id = false, bad_v = false;
  float wmax = 0.f;
  for (int c = lane; c < k; c += G) {
    const float w = L.W[(int64_t)c * L.ld_w + i];
    if (!(w >= 0.f) || isinf(w)) bad_v = true;
    else wmax = fmaxf(wmax, w);
  }
#pragma unroll
  for (int s = 1; s < G; s <<= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, s, G));
  for (int c = lane; c < k; c += G) {
    const float w = L.W[(int64_t)c * L.ld_w + i];
    const int32_t j = L.idx[(int64_t)c * L.ld + i];
    uint32_t q = 0u;
    float2 yj = make_float2(0.f, 0.f);
    if (j < 1 || (int64_t)j > L.N) {
      bad_id = true;
    } else {
      yj = L.Yt[j - 1];
      if (w > 0.f && !isinf(w)) {
        const double x = floor((double)w / (double)wmax * 4294967296.0);
        q = x >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)x;
      }
    }
    sQ[c] = q;
    sY[c] = yj;
  }
  const float2 y0 = L.Y[i];
  bad_v |= !isfinite(y0.x) || !isfinite(y0.y);
  if (bad_id) atomicOr(L.status, TR_ST_ID);
  if (bad_v) atomicOr(L.status, TR_ST_VALUE);
  GFICF_WAVE_SYNC();

  float yx = y0.x, yy = y0.y;
  const u64 e0 = (L.qoff + (u64)i) * (u64)k;
  for (int n = L.eb; n < L.ee; ++n) {
    const float alpha = L.lr * (1.f - (float)n / (float)L.n_epochs);
    const u64 kn = uf_mix(L.seed + (u64)n), un = (u64)n;
    for (int base = 0; base < k; base += G) {
      const int c = base + lane;
      bool due = false;
      if (c < k) {
        const u64 qe = (u64)sQ[c];
        due = (((un + 1ull) * qe) >> 32) > ((un * qe) >> 32);
      }
      u64 mask = (__ballot(due) >> lane0) & ((1ull << G) - 1ull);
      while (mask) {                                              // the same in every lane of the group
        const int t = __builtin_ctzll(mask);
        mask &= mask - 1ull;
        const u64 ke = uf_mix(kn + e0 + (u64)(base + t));
        const float2 yj = sY[base + t];                           // one address for the group: a broadcast read
        for (int s0 = 0;; s0 += G) {                              // the first round also applies the attraction
          float2 yn = make_float2(0.f, 0.f);
          if (s0 + lane < L.rate) {
            const u64 key = uf_mix(ke + (u64)(s0 + lane));
            yn = L.Yt[((key >> 32) * (u64)L.N) >> 32];
          }
          if (s0 == 0) uf_attract<T1>(yx, yy, yj.x, yj.y, alpha, L);
          const int cnt = L.rate - s0 < G ? L.rate - s0 : G;
          for (int u = 0; u < cnt; ++u) {
            const float nx = __shfl(yn.x, u, G), ny = __shfl(yn.y, u, G);
            uf_repulse<T1>(yx, yy, nx, ny, alpha, L);
          }
          if (s0 + G >= L.rate) break;
        }
      }
    }
  }
  if (lane == 0) L.Y[i] = make_float2(yx, yy);
}

// ------------------------------------------------------------------------------------------------ vote
// one lane per new cell; its row's labels in LDS ([column][lane]); votes: the lane's own row of the M x C table, zeroed before
__global__ __launch_bounds__(TR_VOTE_THREADS) void k_tr_vote(const int32_t* __restrict__ idx, int64_t ld, const int32_t* __restrict__ labels,
                                                             int64_t N, int64_t M, int k, int C, int32_t* __restrict__ pred,
                                                             int32_t* __restrict__ votes, uint32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int32_t* const lab = reinterpret_cast<int32_t*>(smem) + threadIdx.x;       // lab[c * TR_VOTE_THREADS]
  const int64_t i = (int64_t)blockIdx.x * TR_VOTE_THREADS + threadIdx.x;
  if (i >= M) return;
  bool bad = false;
  for (int c = 0; c < k; ++c) {
    const int32_t j = idx[(int64_t)c * ld + i];
    int32_t l = -1;
    if (j >= 1 && (int64_t)j <= N) l = labels[j - 1];
    if (l < 0 || l >= C) { bad = true; l = -1; }
    lab[c * TR_VOTE_THREADS] = l;
    if (votes && l >= 0) votes[i * C + l] += 1;
  }
  int best = -1, best_n = 0;
  for (int c = 0; c < k; ++c) {
    const int32_t l = lab[c * TR_VOTE_THREADS];
    if (l < 0) continue;
    int n = 0;
    for (int e = 0; e < k; ++e) n += lab[e * TR_VOTE_THREADS] == l ? 1 : 0;
    if (n > best_n) { best_n = n; best = l; }                    // strictly more: among ties the first in the row stays
  }
  pred[i] = best;
  if (bad) atomicOr(status, TR_ST_ID);
}

// ------------------------------------------------------------------------------------------------ boundary conversions (chain)
__global__ __launch_bounds__(256) void k_tr_in(const double* __restrict__ in, int64_t n, float* __restrict__ Y, uint32_t* __restrict__ status) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * n) return;
  const double x = in[(t & 1) * n + (t >> 1)];
  if (!isfinite(x)) atomicOr(status, TR_ST_VALUE);
  Y[t] = (float)x;
}

// ------------------------------------------------------------------------------------------------ checks and stage bodies
int tr_check_table(int64_t N, int64_t M, int k, int64_t ld) {
  if (N < 1 || N > 0x7FFFFFFFll) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld outside [1, 2^31)", (long long)N);
  if (M < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "M = %lld: negative", (long long)M);
  if (k < 1 || k > GFICF_KNN_MAX_K) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %d outside [1, %d]", k, GFICF_KNN_MAX_K);
  if ((int64_t)k > N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %d neighbours asked of N = %lld training rows", k, (long long)N);
  if (N * k >= ((int64_t)1 << 31)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N * k = %lld reaches 2^31", (long long)(N * k));
  if (ld < M) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "leading dimension %lld < M = %lld", (long long)ld, (long long)M);
  return GFICF_OK;
}

int tr_check_search(int64_t N, int64_t M, int d, int k, int metric, int64_t ld) {
  const int rc = tr_check_table(N, M, k, ld);
  if (rc) return rc;
  if (d < 1 || gficf_knn_dpad(d) < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "d = %d outside [1, 128]", d);
  if (!gficf_knn_metric_ok(metric)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "unknown metric %d", metric);
  return GFICF_OK;
}

int tr_check_lc(double lc) {
  if (!(lc >= 1.0) || !(lc <= (double)GFICF_KNN_MAX_K)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "local_connectivity = %g outside [1, %d]", lc, GFICF_KNN_MAX_K);
  return GFICF_OK;
}

int tr_check_layout(int64_t M, int k, double a, double b, double gamma, double lr, int rate, int n_epochs, int eb, int ee, int64_t qoff) {
  if (!(a > 0.0) || !(b > 0.0) || !std::isfinite(a) || !std::isfinite(b)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a = %g, b = %g must be positive", a, b);
  if (!std::isfinite(gamma) || !std::isfinite(lr)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "repulsion_strength / learning_rate not finite");
  if (rate < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative_sample_rate = %d", rate);
  if (n_epochs < 1 || eb < 0 || ee < eb || ee > n_epochs) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "epochs [%d, %d) of %d", eb, ee, n_epochs);
  if (qoff < 0 || qoff > INT64_MAX / k - M) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "query_offset = %lld: (query_offset + M) k must stay below 2^63", (long long)qoff);
  return GFICF_OK;
}

// a workspace is its status word and, for the search, the partial lists behind it
struct TrWs {
  uint32_t* status;
  u64* part;
};
size_t tr_carve(char* base, size_t part_keys, TrWs& w) {
  gficf_carver cv;
  cv.base = base;
  w.status = cv.take<uint32_t>(1);
  w.part = cv.take<u64>(part_keys);
  return cv.total();
}
size_t tr_part_keys(int64_t M, int64_t N, int k) { return (size_t)(M > 0 ? M : 0) * (size_t)tr_split(TR_MAX_CUS, M, N) * (size_t)k; }

// every stage body below enqueues on a status word the caller has zeroed
int tr_search(gficf_ctx* ctx, u64* part, const float* d_train, int64_t N, const float* d_query, int64_t M, int d, int k, int metric, int32_t* d_idx,
              float* d_dist, int64_t ld_out) {
  if (M == 0) return GFICF_OK;
  metric = gficf_knn_search_metric(metric);
  const KnnTileArgs a = knn_plain_args(d_query, M, d_train, N, d, gficf_knn_dpad(d), k, tr_split(ctx->num_cus, M, N), part);
  const int rc = knn_launch_m<false>(ctx, metric, a);
  if (rc) return rc;
  hipLaunchKernelGGL(k_tr_merge, dim3(tr_grid(M, 4)), dim3(256), 0, ctx->stream, (const u64*)part, M, a.S, k, metric, d_idx, d_dist, ld_out);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int tr_weights(gficf_ctx* ctx, uint32_t* status, const int32_t* d_idx, const float* d_dist, int64_t N, int64_t M, int k, int64_t ld, double lc,
               float* d_w, int64_t ld_w, float* d_sigma, float* d_rho) {
  if (M == 0) return GFICF_OK;
  const double cp = lc - 1.0 > 0.0 ? lc - 1.0 : 0.0;
  const int f = (int)std::floor(cp);
  hipLaunchKernelGGL(k_tr_smooth, dim3(tr_grid(M)), dim3(256), 0, ctx->stream, d_idx, d_dist, N, M, k, ld, f, (float)(cp - (double)f), d_w, ld_w,
                     d_sigma, d_rho, status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int tr_plane_finite(gficf_ctx* ctx, uint32_t* status, const float* d_Y_train, int64_t N) {
  hipLaunchKernelGGL(k_addon_finite, dim3(tr_grid(2 * N) < 1024 ? tr_grid(2 * N) : 1024), dim3(256), 0, ctx->stream, d_Y_train, 2 * N, status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int tr_init(gficf_ctx* ctx, uint32_t* status, const int32_t* d_idx, int64_t ld, const float* d_w, int64_t ld_w, const float* d_Y_train, int64_t N,
            int64_t M, int k, float* d_Y) {
  if (M == 0) return GFICF_OK;
  hipLaunchKernelGGL(k_tr_init, dim3(tr_grid(M)), dim3(256), 0, ctx->stream, d_idx, ld, d_w, ld_w, (const float2*)d_Y_train, N, M, k, (float2*)d_Y,
                     status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int tr_layout(gficf_ctx* ctx, uint32_t* status, const int32_t* d_idx, int64_t ld, const float* d_w, int64_t ld_w, const float* d_Y_train, int64_t N,
              int64_t M, int k, float a, float b, float gamma, float lr, int rate, int n_epochs, int eb, int ee, uint64_t seed, int64_t qoff,
              float* d_Y) {
  if (M == 0) return GFICF_OK;
  TrLay L;
  L.idx = d_idx; L.ld = ld; L.W = d_w; L.ld_w = ld_w; L.Yt = (const float2*)d_Y_train; L.N = N; L.M = M; L.k = k;
  L.a = a; L.b = b; L.m2ab = -2.f * a * b; L.g2b = 2.f * gamma * b; L.lr = lr;
  L.rate = rate; L.n_epochs = n_epochs; L.eb = eb; L.ee = ee; L.seed = (u64)seed; L.qoff = (u64)qoff;
  L.Y = (float2*)d_Y; L.status = status;
  const dim3 grid(tr_grid(M, TR_LAY_THREADS / TR_GROUP));
  const size_t lds = tr_layout_lds(k);                            // at most 8 x 128 x 12 B = 12 KiB
  if (a == 1.f && b == 1.f) hipLaunchKernelGGL(k_tr_layout<true>, grid, dim3(TR_LAY_THREADS), lds, ctx->stream, L);
  else hipLaunchKernelGGL(k_tr_layout<false>, grid, dim3(TR_LAY_THREADS), lds, ctx->stream, L);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int tr_vote(gficf_ctx* ctx, uint32_t* status, const int32_t* d_idx, int64_t ld, const int32_t* d_labels, int64_t N, int64_t M, int k, int C,
            int32_t* d_pred, int32_t* d_votes) {
  if (M == 0) return GFICF_OK;
  if (d_votes) GFICF_HIP_CHECK(hipMemsetAsync(d_votes, 0, sizeof(int32_t) * (size_t)M * (size_t)C, ctx->stream));
  hipLaunchKernelGGL(k_tr_vote, dim3(tr_grid(M, TR_VOTE_THREADS)), dim3(TR_VOTE_THREADS), (size_t)k * TR_VOTE_THREADS * sizeof(int32_t), ctx->stream,
                     d_idx, ld, d_labels, N, M, k, C, d_pred, d_votes, status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// the head of a *_device entry: the workspace checked, carved, its status word zeroed
int tr_enter_ws(gficf_ctx* ctx, void* ws, size_t ws_bytes, size_t part_keys, TrWs& w) {
  if (!ws) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL workspace");
  const size_t need = tr_carve(nullptr, part_keys, w);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  tr_carve((char*)ws, part_keys, w);
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), ctx->stream));
  return GFICF_OK;
}

size_t tr_status_only_bytes() {
  TrWs w;
  return tr_carve(nullptr, 0, w);
}

}  // namespace

extern "C" {

int gficf_transform_abi_version(void) { return GFICF_TRANSFORM_ABI_VERSION; }

int gficf_transform_search_split(gficf_ctx* ctx, int64_t M, int64_t N) { return ctx ? tr_split(ctx->num_cus, M, N) : 0; }

size_t gficf_transform_search_workspace_bytes(int64_t M, int64_t N, int k) {
  if (M < 0 || N < 1 || k < 1 || k > GFICF_KNN_MAX_K) return 0;
  TrWs w;
  return tr_carve(nullptr, tr_part_keys(M, N, k), w);
}

int gficf_transform_search_device(gficf_ctx* ctx, const float* d_train, int64_t N, const float* d_query, int64_t M, int d, int k, int metric,
                                  void* ws, size_t ws_bytes, int32_t* d_idx, float* d_dist, int64_t ld_out) {
  GFICF_CTX_ENTER(ctx);
  int rc = tr_check_search(N, M, d, k, metric, ld_out);
  if (rc) return rc;
  if (!d_train || (M > 0 && (!d_query || !d_idx))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  TrWs w;
  rc = tr_enter_ws(ctx, ws, ws_bytes, tr_part_keys(M, N, k), w);
  if (rc) return rc;
  return tr_search(ctx, w.part, d_train, N, d_query, M, d, k, metric, d_idx, d_dist, ld_out);
}

size_t gficf_transform_weights_workspace_bytes(int64_t M, int k) { return (M < 0 || k < 1) ? 0 : tr_status_only_bytes(); }

int gficf_transform_weights_device(gficf_ctx* ctx, const int32_t* d_idx, const float* d_dist, int64_t N, int64_t M, int k, int64_t ld,
                                   double local_connectivity, void* ws, size_t ws_bytes, float* d_w, int64_t ld_w, float* d_sigma, float* d_rho) {
  GFICF_CTX_ENTER(ctx);
  int rc = tr_check_table(N, M, k, ld);
  if (!rc) rc = tr_check_lc(local_connectivity);
  if (rc) return rc;
  if (ld_w < M) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "leading dimension %lld < M = %lld", (long long)ld_w, (long long)M);
  if (M > 0 && (!d_idx || !d_dist || !d_w)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  TrWs w;
  rc = tr_enter_ws(ctx, ws, ws_bytes, 0, w);
  if (rc) return rc;
  return tr_weights(ctx, w.status, d_idx, d_dist, N, M, k, ld, local_connectivity, d_w, ld_w, d_sigma, d_rho);
}

size_t gficf_transform_init_workspace_bytes(int64_t M, int k) { return (M < 0 || k < 1) ? 0 : tr_status_only_bytes(); }

int gficf_transform_init_device(gficf_ctx* ctx, const int32_t* d_idx, int64_t ld, const float* d_w, int64_t ld_w, const float* d_Y_train, int64_t N,
                                int64_t M, int k, void* ws, size_t ws_bytes, float* d_Y) {
  GFICF_CTX_ENTER(ctx);
  int rc = tr_check_table(N, M, k, ld);
  if (rc) return rc;
  if (ld_w < M) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "leading dimension %lld < M = %lld", (long long)ld_w, (long long)M);
  if (!d_Y_train || (M > 0 && (!d_idx || !d_w || !d_Y))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  TrWs w;
  rc = tr_enter_ws(ctx, ws, ws_bytes, 0, w);
  if (!rc) rc = tr_plane_finite(ctx, w.status, d_Y_train, N);
  if (rc) return rc;
  return tr_init(ctx, w.status, d_idx, ld, d_w, ld_w, d_Y_train, N, M, k, d_Y);
}

size_t gficf_transform_layout_workspace_bytes(int64_t M, int k) { return (M < 0 || k < 1) ? 0 : tr_status_only_bytes(); }

int gficf_transform_layout_device(gficf_ctx* ctx, const int32_t* d_idx, int64_t ld, const float* d_w, int64_t ld_w, const float* d_Y_train, int64_t N,
                                  int64_t M, int k, float a, float b, float gamma, float learning_rate, int negative_sample_rate, int n_epochs,
                                  int epoch_begin, int epoch_end, uint64_t seed, int64_t query_offset, float* d_Y, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  int rc = tr_check_table(N, M, k, ld);
  if (!rc) rc = tr_check_layout(M, k, a, b, gamma, learning_rate, negative_sample_rate, n_epochs, epoch_begin, epoch_end, query_offset);
  if (rc) return rc;
  if (ld_w < M) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "leading dimension %lld < M = %lld", (long long)ld_w, (long long)M);
  if (!d_Y_train || (M > 0 && (!d_idx || !d_w || !d_Y))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  TrWs w;
  rc = tr_enter_ws(ctx, ws, ws_bytes, 0, w);
  if (!rc) rc = tr_plane_finite(ctx, w.status, d_Y_train, N);
  if (rc) return rc;
  return tr_layout(ctx, w.status, d_idx, ld, d_w, ld_w, d_Y_train, N, M, k, a, b, gamma, learning_rate, negative_sample_rate, n_epochs, epoch_begin,
                   epoch_end, seed, query_offset, d_Y);
}

size_t gficf_transform_vote_workspace_bytes(int64_t M, int k) { return (M < 0 || k < 1) ? 0 : tr_status_only_bytes(); }

int gficf_transform_vote_device(gficf_ctx* ctx, const int32_t* d_idx, int64_t ld, const int32_t* d_labels, int64_t N, int64_t M, int k, int C,
                                void* ws, size_t ws_bytes, int32_t* d_pred, int32_t* d_votes) {
  GFICF_CTX_ENTER(ctx);
  int rc = tr_check_table(N, M, k, ld);
  if (rc) return rc;
  if (C < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "C = %d classes", C);
  if (!d_labels || (M > 0 && (!d_idx || !d_pred))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  TrWs w;
  rc = tr_enter_ws(ctx, ws, ws_bytes, 0, w);
  if (rc) return rc;
  return tr_vote(ctx, w.status, d_idx, ld, d_labels, N, M, k, C, d_pred, d_votes);
}

int gficf_transform_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  const int rc = gficf_addon_read_status(ctx, ws, &st);
  if (rc) return rc;
  if (st & TR_ST_ID) GFICF_FAIL(GFICF_ERR_BAD_ID, "a neighbour id outside [1, N] or a label outside [0, C)");
  if (st & TR_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "a non-finite distance, membership or coordinate");
  return GFICF_OK;
}

// ------------------------------------------------------------------------------------------------ host forms
namespace {

// the two matrices uploaded and prepared, the table searched: what all three host entries begin with
struct TrHostSearch {
  double *d_X, *d_Q;
  float *d_train, *d_query, *d_dist;
  int32_t* d_idx;
  char* d_sws;
  size_t sws_bytes;
  TrWs sw;
};

void tr_host_search_carve(gficf_carver& cv, TrHostSearch& h, int64_t N, int64_t ld_x, int64_t M, int64_t ld_q, int d, int k) {
  const size_t dpad = (size_t)gficf_knn_dpad(d);
  h.sws_bytes = gficf_transform_search_workspace_bytes(M, N, k);
  h.d_sws = cv.take<char>(h.sws_bytes);                           // first: its head is the status word of the whole chain
  h.d_X = cv.take<double>((size_t)ld_x * (size_t)d);
  h.d_Q = cv.take<double>((size_t)ld_q * (size_t)d);
  h.d_train = cv.take<float>((size_t)N * dpad);
  h.d_query = cv.take<float>((size_t)M * dpad);
  h.d_idx = cv.take<int32_t>((size_t)M * (size_t)k);
  h.d_dist = cv.take<float>((size_t)M * (size_t)k);
}

int tr_host_search_run(gficf_ctx* ctx, gficf_host_io& io, TrHostSearch& h, const double* X_train, int64_t N, int64_t ld_x, const double* Q, int64_t M,
                       int64_t ld_q, int d, int k, int metric) {
  io.up(h.d_X, X_train, sizeof(double) * (size_t)ld_x * (size_t)d);
  io.up(h.d_Q, Q, sizeof(double) * (size_t)ld_q * (size_t)d);
  if (!io.ok()) return GFICF_OK;
  tr_carve(h.d_sws, tr_part_keys(M, N, k), h.sw);
  io.e = hipMemsetAsync(h.sw.status, 0, sizeof(uint32_t), ctx->stream);
  if (!io.ok()) return GFICF_OK;
  int rc = gficf_knn_prepare_device(ctx, h.d_X, 1, N, d, ld_x, metric, h.d_train);
  if (!rc && M > 0) rc = gficf_knn_prepare_device(ctx, h.d_Q, 1, M, d, ld_q, metric, h.d_query);
  if (!rc) rc = tr_search(ctx, h.sw.part, h.d_train, N, h.d_query, M, d, k, metric, h.d_idx, h.d_dist, M > 0 ? M : 1);
  return rc;
}

int tr_check_host(const double* X_train, int64_t N, int64_t ld_x, const double* Q, int64_t M, int64_t ld_q, int d, int k, int metric) {
  const int rc = tr_check_search(N, M, d, k, metric, M);
  if (rc) return rc;
  if (ld_x < N || ld_q < M) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ld_x = %lld < N = %lld or ld_q = %lld < M = %lld", (long long)ld_x, (long long)N,
                                       (long long)ld_q, (long long)M);
  if (!X_train || (M > 0 && !Q)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  return GFICF_OK;
}

}  // namespace

int gficf_transform_search_host(gficf_ctx* ctx, const double* X_train, int64_t N, int64_t ld_x, const double* Q, int64_t M, int64_t ld_q, int d,
                                int k, int metric, int32_t* idx, double* dist) {
  GFICF_CTX_ENTER(ctx);
  int rc = tr_check_host(X_train, N, ld_x, Q, M, ld_q, d, k, metric);
  if (rc) return rc;
  if (M > 0 && !idx) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t mk = (size_t)M * (size_t)k;
  TrHostSearch h{};
  gficf_host_io io{ctx, "gficf_transform_search_host"};
  gficf_carver cv;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    tr_host_search_carve(cv, h, N, ld_x, M, ld_q, d, k);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  std::vector<float> hd;
  if (io.ok()) {
    rc = tr_host_search_run(ctx, io, h, X_train, N, ld_x, Q, M, ld_q, d, k, metric);
    if (!rc) io.down(idx, h.d_idx, sizeof(int32_t) * mk);
    if (!rc && dist) {
      hd.resize(mk);
      io.down(hd.data(), h.d_dist, sizeof(float) * mk);
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  rc = gficf_transform_sync(ctx, h.d_sws);
  if (rc) return rc;
  if (dist)
    for (size_t t = 0; t < mk; ++t) dist[t] = (double)hd[t];
  return GFICF_OK;
}

int gficf_transform_host(gficf_ctx* ctx, const double* X_train, int64_t N, int64_t ld_x, const double* Y_train, const double* Q, int64_t M,
                         int64_t ld_q, int d, int metric, int k, double local_connectivity, double a, double b, double gamma, double learning_rate,
                         int negative_sample_rate, int n_epochs, int epoch_begin, int epoch_end, const double* init, uint64_t seed,
                         int64_t query_offset, double* embedding, int32_t* idx, float* dist, float* w, float* sigma, float* rho, double* y0) {
  GFICF_CTX_ENTER(ctx);
  int rc = tr_check_host(X_train, N, ld_x, Q, M, ld_q, d, k, metric);
  if (!rc) rc = tr_check_lc(local_connectivity);
  if (!rc) rc = tr_check_layout(M, k, a, b, gamma, learning_rate, negative_sample_rate, n_epochs, epoch_begin, epoch_end, query_offset);
  if (rc) return rc;
  if (!Y_train || (M > 0 && !embedding)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t mk = (size_t)M * (size_t)k;
  TrHostSearch h{};
  double *d_Yt64, *d_init, *d_emb, *d_y0;
  float *d_Yt, *d_Y, *d_w, *d_sigma, *d_rho;
  gficf_host_io io{ctx, "gficf_transform_host"};
  gficf_carver cv;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    tr_host_search_carve(cv, h, N, ld_x, M, ld_q, d, k);
    d_Yt64 = cv.take<double>(2 * (size_t)N); d_init = cv.take<double>(2 * (size_t)M); d_emb = cv.take<double>(2 * (size_t)M);
    d_y0 = cv.take<double>(2 * (size_t)M);
    d_Yt = cv.take<float>(2 * (size_t)N); d_Y = cv.take<float>(2 * (size_t)M); d_w = cv.take<float>(mk);
    d_sigma = cv.take<float>((size_t)M); d_rho = cv.take<float>((size_t)M);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_Yt64, Y_train, sizeof(double) * 2 * (size_t)N);
  if (init) io.up(d_init, init, sizeof(double) * 2 * (size_t)M);
  if (io.ok()) {
    hipStream_t st = ctx->stream;
    const int64_t ld = M > 0 ? M : 1;
    rc = tr_host_search_run(ctx, io, h, X_train, N, ld_x, Q, M, ld_q, d, k, metric);
    uint32_t* const status = h.sw.status;                         // one status word: what gficf_transform_sync(ctx, d_sws) reads
    if (!rc && io.ok()) {
      hipLaunchKernelGGL(k_tr_in, dim3(tr_grid(2 * N)), dim3(256), 0, st, (const double*)d_Yt64, N, d_Yt, status);
      rc = tr_weights(ctx, status, h.d_idx, h.d_dist, N, M, k, ld, local_connectivity, d_w, ld, d_sigma, d_rho);
    }
    if (!rc && io.ok() && M > 0) {
      if (init) hipLaunchKernelGGL(k_tr_in, dim3(tr_grid(2 * M)), dim3(256), 0, st, (const double*)d_init, M, d_Y, status);
      else rc = tr_init(ctx, status, h.d_idx, ld, d_w, ld, d_Yt, N, M, k, d_Y);
      if (!rc && y0) {
        hipLaunchKernelGGL(k_addon_out, dim3(tr_grid(2 * M)), dim3(256), 0, st, (const float*)d_Y, M, d_y0);
        io.down(y0, d_y0, sizeof(double) * 2 * (size_t)M);
      }
      if (!rc)
        rc = tr_layout(ctx, status, h.d_idx, ld, d_w, ld, d_Yt, N, M, k, (float)a, (float)b, (float)gamma, (float)learning_rate,
                       negative_sample_rate, n_epochs, epoch_begin, epoch_end, seed, query_offset, d_Y);
      if (!rc) {
        hipLaunchKernelGGL(k_addon_out, dim3(tr_grid(2 * M)), dim3(256), 0, st, (const float*)d_Y, M, d_emb);
        if (io.ok()) io.e = hipGetLastError();
        io.down(embedding, d_emb, sizeof(double) * 2 * (size_t)M);
        if (idx) io.down(idx, h.d_idx, sizeof(int32_t) * mk);
        if (dist) io.down(dist, h.d_dist, sizeof(float) * mk);
        if (w) io.down(w, d_w, sizeof(float) * mk);
        if (sigma) io.down(sigma, d_sigma, sizeof(float) * (size_t)M);
        if (rho) io.down(rho, d_rho, sizeof(float) * (size_t)M);
      }
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_transform_sync(ctx, h.d_sws);
}

int gficf_transform_classify_host(gficf_ctx* ctx, const double* X_train, int64_t N, int64_t ld_x, const double* Q, int64_t M, int64_t ld_q, int d,
                                  int k, int metric, const int32_t* labels, int C, int32_t* pred) {
  GFICF_CTX_ENTER(ctx);
  int rc = tr_check_host(X_train, N, ld_x, Q, M, ld_q, d, k, metric);
  if (rc) return rc;
  if (C < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "C = %d classes", C);
  if (!labels || (M > 0 && !pred)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  TrHostSearch h{};
  int32_t *d_labels, *d_pred;
  gficf_host_io io{ctx, "gficf_transform_classify_host"};
  gficf_carver cv;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    tr_host_search_carve(cv, h, N, ld_x, M, ld_q, d, k);
    d_labels = cv.take<int32_t>((size_t)N); d_pred = cv.take<int32_t>((size_t)M);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_labels, labels, sizeof(int32_t) * (size_t)N);
  if (io.ok()) {
    rc = tr_host_search_run(ctx, io, h, X_train, N, ld_x, Q, M, ld_q, d, k, metric);
    if (!rc && io.ok()) rc = tr_vote(ctx, h.sw.status, h.d_idx, M > 0 ? M : 1, d_labels, N, M, k, C, d_pred, nullptr);
    if (!rc) io.down(pred, d_pred, sizeof(int32_t) * (size_t)M);
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_transform_sync(ctx, h.d_sws);
}

}  // extern "C"
