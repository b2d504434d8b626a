// gsea.hip — gene-set enrichment of every cluster's gene ranking: the per-cluster fgsea call of runGSEA() (reference
// R/pathwayAnalisys.R:65-96, fgsea at gseaParam = 0) for all clusters and pathways at once.  Built into libgficf_gsea.so, which
// links libgficf_hip.so and uses its context, pool, radix sort and error plumbing (include/gficf_gsea.h states the contract).
//
// At gseaParam = 0 every weight is 1: the score of a set depends only on the positions of its members in the cluster's ordering
// of the genes, and its permutation null only on (G, set size).  One null table (nsim values per distinct size) serves every
// pathway of that size in every cluster.  A set of positions is a bit mask of G bits in LDS and its running sum a popcount scan,
// so one walker scores the observed sets and the random ones, without a sort per set.  Launches, all on the context's stream:
//   (addon_sort.h)   k_sort_keys: order-preserving descending 64-bit key of every statistic (-0.0 -> +0.0; NaN / Inf flagged);
//                    3 radix sorts, stable LSD by the key's low 32 bits, its high 32 bits, then the cluster (k_sort_next
//                    between them): (cluster, statistic desc, row) order
//   k_gs_rank        r_c(g), the position of gene g in cluster c's order
//   k_gs_es<false>   one workgroup per (pathway, cluster): the observed ES
//   per batch of B permutations:
//     k_gs_perm_keys (key_j(g), j, g); 2 radix sorts: by the 32-bit key, then (k_sort_next<1>) stably by the batch-local j
//                    -> the rows pi_j
//     k_gs_es<true>  one workgroup per (size, permutation): null[d][j], the ES of the first m entries of pi_j
//   k_gs_null_sums   per size: the counts and fixed-order sums of its null row
//   k_gs_stats       one wave per (pathway, cluster): the counts against its size's null row, NES and pval
#include <algorithm>
#include <cmath>
#include <vector>

#include "addon_sort.h"
#include "addon_status.h"
#include "common.h"
#include "gficf_gsea.h"

namespace {

typedef unsigned long long u64;

constexpr int GS_MAX_WORDS = GFICF_GSEA_MAX_G / 32;   // the LDS mask: 16 KiB
constexpr int64_t GS_BATCH_ELEMS = (int64_t)1 << 22;  // (permutation, gene) pairs of one batch
constexpr int64_t GS_BATCH_MAX = 1024;                // permutations of one batch
constexpr uint32_t GS_ST_VALUE = 1u;                  // a NaN or infinite statistic
constexpr uint32_t GS_ST_RANGE = 2u;                  // a member outside [0, G)
constexpr uint32_t GS_ST_DUP = 4u;                    // a member repeated within a tested pathway
constexpr uint32_t GS_ST_SIZE = 8u;                   // a size index that does not name the pathway's length

struct GsNull {                                       // per distinct size, over its null row
  int64_t n_ge_zero, n_le_zero;
  double ge_zero_mean, le_zero_mean;
};

__host__ __device__ inline uint32_t gs_mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

// sorted position i holds statistic val[i] = c * G + g; every cluster has G of them, so cluster c fills [c * G, (c + 1) * G)
__global__ __launch_bounds__(256) void k_gs_rank(int64_t n, uint32_t G, const uint32_t* __restrict__ val, int32_t* __restrict__ rank) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t p = val[i];
    if ((int64_t)p < n) rank[p] = (int32_t)(i - (int64_t)(p / G) * G);
  }
}

// element jb * G + g of the batch: key_(j0 + jb)(g)
__global__ __launch_bounds__(256) void k_gs_perm_keys(int64_t n, uint32_t G, uint32_t seed_mix, uint32_t j0, u64* __restrict__ kv) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t jb = (uint32_t)i / G, g = (uint32_t)i - jb * G;
    const uint32_t cj = gs_mix32(j0 + jb + seed_mix);
    kv[i] = ((u64)gs_mix32(g ^ cj) << 32) | (u64)i;
  }
}

// The walker.  A workgroup per set: the members' positions as bits of an LDS mask, the popcounts of the mask's words scanned
// across the workgroup (thread t owns the words [t * wpt, (t + 1) * wpt), wpt odd so that the threads' words fall into
// different banks), every thread walks the set bits of its words with the ordinal i the scan gave it, max top / min bottom
// reduced over the workgroup.
//   NUL = false: block b = pathway x + nx * cluster y; members r_y(row) of pathway x; out = es[b]
//   NUL = true:  block b = size x + nx * batch-local permutation y; members perm[y * G + 0 .. m - 1] - y * G; out = null[x * nsim + j0 + y]
template <bool NUL>
__global__ __launch_bounds__(256) void k_gs_es(int32_t G, int64_t nx, int32_t D, const int32_t* __restrict__ sizes, const int32_t* __restrict__ size_idx,
                                               const int64_t* __restrict__ ptr, int64_t n_members, const int32_t* __restrict__ members,
                                               const int32_t* __restrict__ rank, const uint32_t* __restrict__ perm, int64_t nsim, int64_t j0,
                                               double* __restrict__ out, uint32_t* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ uint32_t s_mask[GS_MAX_WORDS];
  __shared__ int32_t s_cnt[4];
  __shared__ double s_max[4], s_min[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t x = (int64_t)blockIdx.x % nx, y = (int64_t)blockIdx.x / nx;
  int32_t m;
  int64_t beg = 0;
  double* o;
  if (NUL) {
    m = sizes[x];
    o = out + x * nsim + j0 + y;
    if (m < 1 || m >= G) {                                 // (not a size the contract allows: GS_ST_SIZE is raised by the observed walk or the host)
      if (t == 0) { *o = 0.0; atomicOr(status, GS_ST_SIZE); }
      return;
    }
  } else {
    o = out + blockIdx.x;
    const int32_t d = size_idx[x];
    beg = ptr[x];
    const int64_t len = ptr[x + 1] - beg;
    if (d < 0) {                                           // not tested
      if (t == 0) *o = 0.0;
      return;
    }
    if (d >= D || beg < 0 || len < 1 || len >= G || beg + len > n_members || (int64_t)sizes[d] != len) {
      if (t == 0) { *o = 0.0; atomicOr(status, GS_ST_SIZE); }
      return;
    }
    m = (int32_t)len;
  }
  const int W = (G + 31) >> 5;
  for (int w = t; w < W; w += 256) s_mask[w] = 0u;
  __syncthreads();
  for (int k = t; k < m; k += 256) {
    uint32_t pos;
    if (NUL) {
      pos = perm[y * G + k] - (uint32_t)(y * G);
    } else {
      const int32_t row = members[beg + k];
      if (row < 0 || row >= G) { atomicOr(status, GS_ST_RANGE); continue; }
      pos = (uint32_t)rank[y * G + row];
    }
    if (pos < (uint32_t)G) atomicOr(&s_mask[pos >> 5], 1u << (pos & 31));
  }
  __syncthreads();
  const int wpt = ((W + 255) >> 8) | 1;
  const int w0 = t * wpt < W ? t * wpt : W, w1 = w0 + wpt < W ? w0 + wpt : W;
  int32_t cnt = 0;
  for (int w = w0; w < w1; ++w) cnt += __popc(s_mask[w]);
  int32_t incl = cnt;                                      // inclusive scan over the wave, then the waves' totals through LDS
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) s_cnt[wave] = incl;
  __syncthreads();
  int32_t i = incl - cnt, total = 0;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    if (v < wave) i += s_cnt[v];
    total += s_cnt[v];
  }
  if (!NUL && t == 0 && total != m) atomicOr(status, GS_ST_DUP);
  const double dm = (double)m, dgm = (double)(G - m), inv_m = 1.0 / dm;
  double mx = -INFINITY, mn = INFINITY;
  for (int w = w0; w < w1; ++w) {
    uint32_t bits = s_mask[w];
    while (bits) {
      const int32_t S = (w << 5) + __builtin_ctz(bits) + 1;    // 1-based position
      bits &= bits - 1u;
      ++i;
      const double top = (double)i / dm - (double)(S - i) / dgm;
      const double bottom = top - inv_m;
      mx = fmax(mx, top);
      mn = fmin(mn, bottom);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mx = fmax(mx, __shfl_xor(mx, d));
    mn = fmin(mn, __shfl_xor(mn, d));
  }
  if (lane == 0) { s_max[wave] = mx; s_min[wave] = mn; }
  __syncthreads();
  if (t == 0) {
    const double maxP = fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3]));
    const double minP = fmin(fmin(s_min[0], s_min[1]), fmin(s_min[2], s_min[3]));
    *o = maxP > -minP ? maxP : (maxP < -minP ? minP : 0.0);
  }
}

// One workgroup per size.  Thread t adds x_t, x_(t + 256), ... in turn; the 256 partial sums are folded t with t + 128, + 64, ... + 1.
__global__ __launch_bounds__(256) void k_gs_null_sums(int64_t nsim, const double* __restrict__ null, GsNull* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double s_ge[256], s_le[256];
  __shared__ int64_t s_nge[256], s_nle[256];
  const int t = threadIdx.x;
  const double* row = null + (int64_t)blockIdx.x * nsim;
  double ge = 0.0, le = 0.0;
  int64_t nge = 0, nle = 0;
  for (int64_t j = t; j < nsim; j += 256) {
    const double x = row[j];
    if (x >= 0.0) { ++nge; ge += x; }
    if (x <= 0.0) { ++nle; le += x; }
  }
  s_ge[t] = ge; s_le[t] = le; s_nge[t] = nge; s_nle[t] = nle;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (t < h) { s_ge[t] += s_ge[t + h]; s_le[t] += s_le[t + h]; s_nge[t] += s_nge[t + h]; s_nle[t] += s_nle[t + h]; }
    __syncthreads();
  }
  if (t == 0) {
    GsNull o;
    o.n_ge_zero = s_nge[0]; o.n_le_zero = s_nle[0];
    o.ge_zero_mean = s_ge[0] / (double)s_nge[0];
    o.le_zero_mean = s_le[0] / (double)s_nle[0];
    out[blockIdx.x] = o;
  }
}

// one wave per (pathway, cluster), pathway fastest
__global__ __launch_bounds__(256) void k_gs_stats(int64_t P, int64_t total, int32_t D, int64_t nsim, const int32_t* __restrict__ size_idx,
                                                  const double* __restrict__ null, const GsNull* __restrict__ nsum, const double* __restrict__ es,
                                                  double* __restrict__ nes, double* __restrict__ pval) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  for (int64_t q = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6; q < total; q += ((int64_t)gridDim.x * 256) >> 6) {
    const int32_t d = size_idx[q % P];
    if (d < 0 || d >= D) {
      if (lane == 0) { nes[q] = 0.0; pval[q] = 0.0; }
      continue;
    }
    const double e = es[q];
    const double* row = null + (int64_t)d * nsim;
    int64_t nge = 0, nle = 0;
    for (int64_t j = lane; j < nsim; j += 64) {
      const double x = row[j];
      nge += x >= e ? 1 : 0;
      nle += x <= e ? 1 : 0;
    }
    nge = gficf_wave_sum(nge);
    nle = gficf_wave_sum(nle);
    if (lane == 0) {
      const GsNull s = nsum[d];
      nes[q] = e / (e > 0.0 ? s.ge_zero_mean : fabs(s.le_zero_mean));
      pval[q] = fmin((double)(1 + nle) / (double)(1 + s.n_le_zero), (double)(1 + nge) / (double)(1 + s.n_ge_zero));
    }
  }
}

// ------------------------------------------------------- workspace
struct GsWs {
  uint32_t* status;
  gficf_sort_bufs sort;
  int32_t* rank;
  GsNull* nsum;
  double* null;
};

static int64_t gs_batch(int64_t G, int64_t nsim) {
  if (G < 1 || nsim < 1) return 0;
  int64_t b = GS_BATCH_ELEMS / G;
  if (b > GS_BATCH_MAX) b = GS_BATCH_MAX;
  if (b > nsim) b = nsim;
  return b > 1 ? b : 1;
}

static size_t gs_carve(char* base, int64_t G, int64_t C, int64_t D, int64_t nsim, GsWs& w) {
  gficf_carver cv;
  cv.base = base;
  const int64_t gc = G * C, bg = gs_batch(G, nsim) * G, nmax = std::max<int64_t>(std::max(gc, bg), 1);
  w.status = cv.take<uint32_t>(1);
  // the statistics have 64-bit keys, a batch of permutations has the more elements; the cluster and the batch-local j are groups
  w.sort.take(cv, (size_t)std::max<int64_t>(gc, 1), (size_t)nmax, {gficf_bit_width(C - 1), gficf_bit_width(GS_BATCH_MAX - 1)});
  w.rank = cv.take<int32_t>((size_t)std::max<int64_t>(gc, 1));
  w.nsum = cv.take<GsNull>((size_t)std::max<int64_t>(D, 1));
  w.null = cv.take<double>((size_t)std::max<int64_t>(D * nsim, 1));
  return cv.total();
}

static int gs_check_sizes(int64_t G, int64_t C, int64_t P, int64_t n_members, int64_t D, int64_t nsim) {
  if (G < 1 || C < 1 || P < 0 || n_members < 0 || D < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, C = %lld, P = %lld: a size is out of range", (long long)G, (long long)C, (long long)P);
  if (nsim < 1 || nsim > INT32_MAX) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "nsim = %lld: at least one permutation (and at most 2^31 - 1)", (long long)nsim);
  if (G > GFICF_GSEA_MAX_G) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "G = %lld genes: the LDS gene mask holds %d", (long long)G, GFICF_GSEA_MAX_G);
  if (G * C > INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^31 - 1 statistics");
  if ((double)P * (double)C > (double)INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^31 - 1 (pathway, cluster) pairs");
  if (D >= G && D > 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "D = %lld distinct sizes, but the sizes lie in [1, G - 1]", (long long)D);
  return GFICF_OK;
}

// the rows pi_(j0) ... pi_(j0 + bc - 1) into s.oval (row jb at [jb * G, (jb + 1) * G), its entries offset by jb * G)
static int gs_permutations(gficf_ctx* ctx, const gficf_sort_bufs& s, int64_t G, uint32_t seed, int64_t j0, int64_t bc) {
  hipStream_t st = ctx->stream;
  const int64_t n = bc * G;
  hipLaunchKernelGGL(k_gs_perm_keys, dim3(gficf_grid_1d(n)), dim3(256), 0, st, n, (uint32_t)G, gs_mix32(seed), (uint32_t)j0, s.kv0);
  GFICF_HIP_CHECK(hipGetLastError());
  int rc = gficf_radix_sort_kv(ctx, s.kv0, s.kv1, s.hist, n, 32, s.okey, s.oval);                   // the 32-bit key
  if (rc || bc == 1) return rc;
  hipLaunchKernelGGL(k_sort_next<1>, dim3(gficf_grid_1d(n)), dim3(256), 0, st, n, (const uint32_t*)s.oval, (const u64*)nullptr, (const uint32_t*)nullptr,
                     (uint32_t)G, s.kv0);
  GFICF_HIP_CHECK(hipGetLastError());
  return gficf_radix_sort_kv(ctx, s.kv0, s.kv1, s.hist, n, gficf_bit_width(bc - 1), s.okey, s.oval);   // the batch-local j, stably
}

}  // namespace

extern "C" {

int gficf_gsea_abi_version(void) { return GFICF_GSEA_ABI_VERSION; }

int64_t gficf_gsea_perm_batch(int64_t G, int64_t nsim) { return gs_batch(G, nsim); }

size_t gficf_gsea_workspace_bytes(int64_t G, int32_t C, int64_t P, int64_t n_members, int32_t D, int64_t nsim) {
  if (G < 1 || C < 1 || P < 0 || n_members < 0 || D < 0 || nsim < 1 || G > GFICF_GSEA_MAX_G || G * (int64_t)C > INT32_MAX) return 0;
  GsWs w;
  return gs_carve(nullptr, G, C, D, nsim, w);
}

int gficf_gsea_device(gficf_ctx* ctx, int64_t G, int32_t C, const double* d_stats, int64_t P, const int64_t* d_ptr, const int32_t* d_members,
                      int64_t n_members, int32_t D, const int32_t* d_sizes, const int32_t* d_size_idx, int64_t nsim, uint32_t seed, void* ws,
                      size_t ws_bytes, double* d_es, double* d_nes, double* d_pval, double* d_null) {
  GFICF_CTX_ENTER(ctx);
  int rc = gs_check_sizes(G, C, P, n_members, D, nsim);
  if (rc) return rc;
  if (!d_stats || !d_ptr || !ws || (P > 0 && (!d_size_idx || !d_es || !d_nes || !d_pval)) || (n_members > 0 && !d_members) || (D > 0 && !d_sizes))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  GsWs w;
  rc = gficf_addon_carve(ws, ws_bytes, [&](char* base) { return gs_carve(base, G, C, D, nsim, w); });
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), st));
  if (P == 0) return GFICF_OK;
  const int64_t gc = G * C;
  rc = gficf_sort_f64(ctx, w.sort, gc, {d_stats, 1, nullptr, w.status, GS_ST_VALUE, nullptr, nullptr, (uint32_t)G, gficf_bit_width(C - 1)});   // (cluster, statistic desc, row) order
  if (rc) return rc;
  hipLaunchKernelGGL(k_gs_rank, dim3(gficf_grid_1d(gc)), dim3(256), 0, st, gc, (uint32_t)G, (const uint32_t*)w.sort.oval, w.rank);
  hipLaunchKernelGGL(k_gs_es<false>, dim3((unsigned)(P * C)), dim3(256), 0, st, (int32_t)G, P, D, d_sizes, d_size_idx, d_ptr, n_members, d_members,
                     (const int32_t*)w.rank, (const uint32_t*)nullptr, nsim, (int64_t)0, d_es, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  double* const null = d_null ? d_null : w.null;
  if (D > 0) {
    const int64_t B = gs_batch(G, nsim);
    for (int64_t j0 = 0; j0 < nsim; j0 += B) {
      const int64_t bc = nsim - j0 < B ? nsim - j0 : B;
      rc = gs_permutations(ctx, w.sort, G, seed, j0, bc);
      if (rc) return rc;
      hipLaunchKernelGGL(k_gs_es<true>, dim3((unsigned)(D * bc)), dim3(256), 0, st, (int32_t)G, (int64_t)D, D, d_sizes, (const int32_t*)nullptr,
                         (const int64_t*)nullptr, (int64_t)0, (const int32_t*)nullptr, (const int32_t*)nullptr, (const uint32_t*)w.sort.oval, nsim, j0, null,
                         w.status);
      GFICF_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_gs_null_sums, dim3((unsigned)D), dim3(256), 0, st, nsim, (const double*)null, w.nsum);
  }
  hipLaunchKernelGGL(k_gs_stats, dim3(gficf_grid_1d(P * C * 64)), dim3(256), 0, st, P, P * C, D, nsim, d_size_idx, (const double*)null, (const GsNull*)w.nsum,
                     (const double*)d_es, d_nes, d_pval);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_gsea_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  const int rc = gficf_addon_read_status(ctx, ws, &st);
  if (rc) return rc;
  if (st & GS_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "the statistics hold a NaN or an infinite value");
  if (st & GS_ST_RANGE) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a pathway member outside [0, G)");
  if (st & GS_ST_DUP) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a member repeated within a pathway");
  if (st & GS_ST_SIZE) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a size index that does not name its pathway's length, or a size outside [1, G - 1]");
  return GFICF_OK;
}

int gficf_gsea_host(gficf_ctx* ctx, int64_t G, int32_t C, const double* stats, int64_t P, const int64_t* ptr, const int32_t* members, int64_t nsim,
                    uint32_t seed, int64_t min_size, int64_t max_size, double* es, double* nes, double* pval, double* null, int64_t null_rows) {
  GFICF_CTX_ENTER(ctx);
  if (P < 0 || !ptr) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "P = %lld pathways, ptr = %p", (long long)P, (const void*)ptr);
  if (ptr[0] != 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ptr[0] = %lld, expected 0", (long long)ptr[0]);
  for (int64_t p = 0; p < P; ++p)
    if (ptr[p + 1] < ptr[p]) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ptr decreases at position %lld", (long long)(p + 1));
  const int64_t nm = ptr[P];
  const int64_t hi = max_size < G - 1 ? max_size : G - 1, lo = min_size > 1 ? min_size : 1;
  std::vector<int32_t> sizes, sidx((size_t)(P > 0 ? P : 1), -1);
  for (int64_t p = 0; p < P; ++p) {
    const int64_t m = ptr[p + 1] - ptr[p];
    if (m >= lo && m <= hi) sizes.push_back((int32_t)m);
  }
  std::sort(sizes.begin(), sizes.end());
  sizes.erase(std::unique(sizes.begin(), sizes.end()), sizes.end());
  for (int64_t p = 0; p < P; ++p) {
    const int64_t m = ptr[p + 1] - ptr[p];
    if (m >= lo && m <= hi) sidx[(size_t)p] = (int32_t)(std::lower_bound(sizes.begin(), sizes.end(), (int32_t)m) - sizes.begin());
  }
  const int64_t D = (int64_t)sizes.size();
  int rc = gs_check_sizes(G, C, P, nm, D, nsim);
  if (rc) return rc;
  if (!stats || (P > 0 && (!es || !nes || !pval)) || (nm > 0 && !members)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  if (null && null_rows != D) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "null has %lld rows, but %lld distinct sizes are tested", (long long)null_rows, (long long)D);
  const size_t gc = (size_t)(G * C), pc = (size_t)(P * C), dn = (size_t)(D * nsim);
  const size_t wsb = gficf_gsea_workspace_bytes(G, C, P, nm, (int32_t)D, nsim);
  gficf_host_io io{ctx, "gficf_gsea_host"};
  gficf_carver cv;
  double *d_st, *d_es, *d_nes, *d_pv, *d_nu; int64_t* d_ptr; int32_t *d_mem, *d_sz, *d_si; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_st = cv.take<double>(gc); d_ptr = cv.take<int64_t>((size_t)P + 1); d_mem = cv.take<int32_t>((size_t)(nm > 0 ? nm : 1));
    d_sz = cv.take<int32_t>((size_t)(D > 0 ? D : 1)); d_si = cv.take<int32_t>(sidx.size());
    d_es = cv.take<double>(pc ? pc : 1); d_nes = cv.take<double>(pc ? pc : 1); d_pv = cv.take<double>(pc ? pc : 1);
    d_nu = cv.take<double>(null && dn ? dn : 1);
    d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_st, stats, sizeof(double) * gc);
  io.up(d_ptr, ptr, sizeof(int64_t) * ((size_t)P + 1));
  io.up(d_mem, members, sizeof(int32_t) * (size_t)nm);
  io.up(d_sz, sizes.data(), sizeof(int32_t) * (size_t)D);
  io.up(d_si, sidx.data(), sizeof(int32_t) * (size_t)P);
  if (io.ok()) {
    rc = gficf_gsea_device(ctx, G, C, d_st, P, d_ptr, d_mem, nm, (int32_t)D, d_sz, d_si, nsim, seed, d_ws, wsb, d_es, d_nes, d_pv, null ? d_nu : nullptr);
    if (!rc) {
      io.down(es, d_es, sizeof(double) * pc);
      io.down(nes, d_nes, sizeof(double) * pc);
      io.down(pval, d_pv, sizeof(double) * pc);
      if (null) io.down(null, d_nu, sizeof(double) * dn);
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_gsea_sync(ctx, d_ws);
}

int gficf_gsea_permutation_host(gficf_ctx* ctx, int64_t G, uint32_t seed, int64_t j, int32_t* out) {
  GFICF_CTX_ENTER(ctx);
  if (G < 1 || j < 0 || j > (int64_t)UINT32_MAX || !out) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, j = %lld, out = %p", (long long)G, (long long)j, (void*)out);
  if (G > GFICF_GSEA_MAX_G) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "G = %lld genes: the LDS gene mask holds %d", (long long)G, GFICF_GSEA_MAX_G);
  gficf_host_io io{ctx, "gficf_gsea_permutation_host"};
  gficf_carver cv;
  gficf_sort_bufs s;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    s.take(cv, 0, (size_t)G, {});                          // no 64-bit keys: one pass over the 32-bit ones
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  int rc = GFICF_OK;
  if (io.ok()) {
    rc = gs_permutations(ctx, s, G, seed, j, 1);
    if (!rc) io.down(out, s.oval, sizeof(int32_t) * (size_t)G);
  }
  return io.finish(rc);
}

}  // extern "C"
