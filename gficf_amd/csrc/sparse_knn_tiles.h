// sparse_knn_tiles.h — the tile kernel of the exact kNN search over sparse cells, as text: its constants and shape rules, the
// prepare pass, the tile kernel (dense queries in LDS, sparse candidates streamed), the merge and the TQ dispatch.  Two objects
// include it: sparse_knn.hip (queries are a column range of the same matrix, SELF = true: include/gficf_sparse_knn.h) and
// sparse_query.hip (queries are the columns of a second matrix, SELF = false: include/gficf_sparse_query.h).  It depends on no
// flag that differs between them: both are compiled with -ffp-contract=off.
#pragma once

#include "gficf_sparse_knn.h"

#include "addon_status.h"

namespace {

constexpr int SK_LANES = GFICF_SPARSE_KNN_LANES;          // lanes of the group that walks one column
constexpr int SK_THREADS = 512;                           // tile workgroup: 8 waves, one per query of the widest tile
constexpr int SK_WAVES = SK_THREADS / 64;
constexpr int SK_GROUPS = SK_THREADS / SK_LANES;          // candidates in flight
constexpr int SK_ROUND = 2;                               // candidates a group takes between two barriers
constexpr int SK_STAGE = SK_GROUPS * SK_ROUND;            // candidates per round: the hand-over slots of one query
constexpr int SK_UNROLL = 4;                              // entries of a chain loaded ahead of their use
constexpr int SK_MAX_TQ = 8;
constexpr int64_t SK_MAX_G = GFICF_SPARSE_KNN_LDS_FLOATS;
constexpr int SK_CUS = 256;                               // workgroups that fill the chip (one 128 KiB tile per CU)
constexpr int SK_MAX_SLICES = 32;
constexpr int64_t SK_MIN_SLICE = 256;                     // candidates a slice holds at least
constexpr int SK_MERGE_THREADS = 256;
constexpr unsigned long long SK_SENTINEL = ~0ull;
constexpr uint32_t SK_ST_CSC = 1u, SK_ST_VALUE = 2u;

static_assert(SK_WAVES >= SK_MAX_TQ, "one wave keeps one query's list");
static_assert(SK_MAX_G * 4 + SK_MAX_TQ * (GFICF_KNN_MAX_K + SK_STAGE) * 8 + 64 <= 160 * 1024 - 64, "the tile's LDS");

typedef unsigned long long u64;

// ---------------------------------------------------------------- shape
int sk_tile_queries(int64_t G) {
  for (int tq = SK_MAX_TQ; tq > 1; tq >>= 1)
    if (G * tq <= SK_MAX_G) return tq;
  return 1;
}

// the candidate slices for n_q queries against N cells
int sk_slices(int64_t n_q, int64_t N, int tq) {
  const int64_t tiles = gficf_ceil_div(n_q, tq);
  if (tiles >= SK_CUS) return 1;
  int64_t s = gficf_ceil_div(SK_CUS, tiles > 0 ? tiles : 1);
  const int64_t room = N / SK_MIN_SLICE;
  if (s > room) s = room;
  if (s > SK_MAX_SLICES) s = SK_MAX_SLICES;
  return s < 1 ? 1 : (int)s;
}

// ---------------------------------------------------------------- device helpers
// the stored entries [b, e) of column c, inside [0, nnz] whatever the pointer holds
__device__ inline void sk_range(const int64_t* colptr, int64_t c, int64_t nnz, int64_t& b, int64_t& e) {
  b = colptr[c];
  e = colptr[c + 1];
  b = b < 0 ? 0 : (b > nnz ? nnz : b);
  e = e < b ? b : (e > nnz ? nnz : e);
}

// the chains of a 16-lane group added in the fixed tree: l with l ^ 8, ^ 4, ^ 2, ^ 1 (every lane ends with the sum)
__device__ inline double sk_tree(double v) {
#pragma unroll
  for (int m = SK_LANES / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__device__ inline uint32_t sk_sortable(float d) {
  const uint32_t u = __float_as_uint(d);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ inline float sk_unsortable(uint32_t s) { return __uint_as_float(s ^ ((s >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// x into the ascending list of k keys one wave keeps (positions lane and lane + 64); the largest key falls off
__device__ inline void sk_insert(u64* list, int k, u64 x, int lane) {
  if (x >= list[k - 1]) return;                               // the same in every lane
  u64 nv[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int p = lane + 64 * h;
    nv[h] = 0;
    if (p < k) {
      const u64 v = list[p];
      if (v < x) nv[h] = v;
      else if (p == 0 || list[p - 1] < x) nv[h] = x;
      else nv[h] = list[p - 1];
    }
  }
  GFICF_WAVE_SYNC();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int p = lane + 64 * h;
    if (p < k) list[p] = nv[h];
  }
  GFICF_WAVE_SYNC();
}

// ---------------------------------------------------------------- prepare
__global__ __launch_bounds__(256) void k_sk_prepare(int64_t G, int64_t N, int64_t nnz, const int64_t* __restrict__ colptr,
                                                    const int32_t* __restrict__ rowidx, const double* __restrict__ x, int metric,
                                                    float* __restrict__ xf, double* __restrict__ p0, double* __restrict__ p1,
                                                    uint32_t* __restrict__ status) {
  const int sl = threadIdx.x & (SK_LANES - 1);
  const int64_t c = (int64_t)blockIdx.x * (256 / SK_LANES) + (threadIdx.x / SK_LANES);
  uint32_t bad = 0;
  double na = 0.0, la = 0.0, sa = 0.0;
  if (c < N) {                                                // (a group is whole inside or outside: N is tested per group)
    const int64_t rb = colptr[c], re = colptr[c + 1];
    if (rb < 0 || re < rb || re > nnz || (c == 0 && rb != 0)) bad |= SK_ST_CSC;
    int64_t b, e;
    sk_range(colptr, c, nnz, b, e);
    for (int64_t p = b + sl; p < e; p += SK_LANES) {
      const int32_t r = rowidx[p];
      if (r < 0 || r >= G || (p > b && rowidx[p - 1] >= r)) bad |= SK_ST_CSC;
      const float v = (float)x[p];
      if (!isfinite(v)) bad |= SK_ST_VALUE;
      xf[p] = v;
      const double a = (double)v;
      na += a * a;
      la += fabs(a);
      sa += a;
    }
  }
  na = sk_tree(na);
  la = sk_tree(la);
  sa = sk_tree(sa);
  if (c < N && sl == 0) {
    double s0 = na, s1 = 0.0;
    if (metric == GFICF_KNN_MANHATTAN) s0 = la;
    else if (metric == GFICF_KNN_COSINE) s0 = sqrt(na);
    else if (metric == GFICF_KNN_CORRELATION) {
      s1 = sa / (double)G;
      const double v = na - (double)G * s1 * s1;
      s0 = v > 0.0 ? sqrt(v) : 0.0;
    }
    p0[c] = s0;
    p1[c] = s1;
  }
  if (bad) atomicOr(status, bad);
}

// ---------------------------------------------------------------- tiles
// the candidates (N cells: colptr .. nnz) and the matrix the queries are columns of (q_colptr .. q_nnz; the same arrays in the
// square search); both have G rows
struct SkArgs {
  int64_t G, N, nnz;
  const int64_t* colptr;
  const int32_t* rowidx;
  const float* xf;
  const double* p0;
  const double* p1;
  int64_t q_nnz;
  const int64_t* q_colptr;
  const int32_t* q_rowidx;
  const float* q_xf;
  const double* q_p0;
  const double* q_p1;
  int k, metric, slices;
  int64_t q_begin, q_end, per_slice;
  u64* part;
};

template <int TQ>
__device__ inline void sk_load_q(const float* q, float (&u)[TQ]) {
  if constexpr (TQ == 8) {
    const float4 a = ((const float4*)q)[0], b = ((const float4*)q)[1];
    u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w; u[4] = b.x; u[5] = b.y; u[6] = b.z; u[7] = b.w;
  } else if constexpr (TQ == 4) {
    const float4 a = ((const float4*)q)[0];
    u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w;
  } else if constexpr (TQ == 2) {
    const float2 a = ((const float2*)q)[0];
    u[0] = a.x; u[1] = a.y;
  } else {
    u[0] = q[0];
  }
}

// the distance of the contract from the pair sum and the two cells' scalars
__device__ inline double sk_distance(int metric, double G, double S, double a0, double a1, double b0, double b1) {
  double d;
  if (metric == GFICF_KNN_EUCLIDEAN) {
    const double v = (a0 + b0) - 2.0 * S;
    d = sqrt(v > 0.0 ? v : 0.0);
  } else if (metric == GFICF_KNN_MANHATTAN) {
    const double v = (a0 + b0) - S;
    d = v > 0.0 ? v : 0.0;
  } else {
    if (a0 == 0.0 || b0 == 0.0) return 1.0;
    const double num = metric == GFICF_KNN_CORRELATION ? S - G * a1 * b1 : S;
    const double v = 1.0 - num / (a0 * b0);
    d = v > 0.0 ? v : 0.0;
  }
  return d;
}

// one stored entry of a candidate (value v) against the TQ query values u of its gene.  The product of two f32 values is exact
// in f64, so the fused multiply-add rounds exactly as the product followed by the add would: one instruction instead of two
template <int TQ, bool MANH>
__device__ inline void sk_visit(const float (&u)[TQ], float v, double (&acc)[TQ]) {
  const double bv = (double)v;
#pragma unroll
  for (int j = 0; j < TQ; ++j) {
    const double av = (double)u[j];
    if constexpr (MANH) acc[j] += (fabs(av) + fabs(bv)) - fabs(av - bv);
    else acc[j] = fma(av, bv, acc[j]);
  }
}

// lane sl's chain of the pair sums of the candidate's entries [b, e): the entries b + sl, b + sl + LANES, ... added in that order.
// SK_UNROLL entries are loaded ahead of their use (global, then LDS) so that their latencies overlap; the adds stay in order.
template <int TQ, bool MANH>
__device__ inline void sk_chain(const SkArgs& a, const float* dense, int G, int64_t b, int64_t e, int sl, double (&acc)[TQ]) {
  int64_t p = b + sl;
  for (; p + (SK_UNROLL - 1) * SK_LANES < e; p += SK_UNROLL * SK_LANES) {
    int32_t r[SK_UNROLL];
    float v[SK_UNROLL], u[SK_UNROLL][TQ];
#pragma unroll
    for (int t = 0; t < SK_UNROLL; ++t) {
      r[t] = a.rowidx[p + t * SK_LANES];
      v[t] = a.xf[p + t * SK_LANES];
    }
#pragma unroll
    for (int t = 0; t < SK_UNROLL; ++t) sk_load_q<TQ>(dense + ((uint32_t)r[t] < (uint32_t)G ? r[t] : 0) * TQ, u[t]);
#pragma unroll
    for (int t = 0; t < SK_UNROLL; ++t) sk_visit<TQ, MANH>(u[t], v[t], acc);
  }
  for (; p < e; p += SK_LANES) {
    const int32_t r = a.rowidx[p];
    float u[TQ];
    sk_load_q<TQ>(dense + ((uint32_t)r < (uint32_t)G ? r : 0) * TQ, u);
    sk_visit<TQ, MANH>(u, a.xf[p], acc);
  }
}

// SELF: the queries are columns of the candidates' matrix and the pair (i, i) gets the distance 0 without arithmetic; without it
// no pair is special and a query id is a column of the query matrix
template <int TQ, bool MANH, bool SELF>
__global__ __launch_bounds__(SK_THREADS) void k_sk_tiles(const SkArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int G = (int)a.G, k = a.k;
  float* const dense = (float*)smem;                                              // [G][TQ]
  u64* const lists = (u64*)(smem + (((size_t)G * TQ * sizeof(float) + 15) & ~(size_t)15));   // [TQ][k]
  u64* const stage = lists + TQ * k;                                              // [TQ][SK_STAGE]
  int* const scnt = (int*)(stage + TQ * SK_STAGE);                               // [TQ]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sl = tid & (SK_LANES - 1), grp = tid / SK_LANES;
  const int64_t q0 = a.q_begin + (int64_t)blockIdx.x * TQ;
  const int nq = (int)(a.q_end - q0 < TQ ? a.q_end - q0 : TQ);
  const int slice = blockIdx.y;

  for (int i = tid; i < G * TQ; i += SK_THREADS) dense[i] = 0.0f;
  for (int i = tid; i < TQ * k; i += SK_THREADS) lists[i] = SK_SENTINEL;
  if (tid < TQ) scnt[tid] = 0;
  __syncthreads();
  if (wave < nq) {                                            // wave j scatters query j
    int64_t b, e;
    sk_range(a.q_colptr, q0 + wave, a.q_nnz, b, e);
    for (int64_t p = b + lane; p < e; p += 64) {
      const int32_t r = a.q_rowidx[p];
      if ((uint32_t)r < (uint32_t)G) dense[r * TQ + wave] = a.q_xf[p];
    }
  }
  __syncthreads();

  double qa0 = 0.0, qa1 = 0.0;                                // lane sl of a group forms the keys of query sl
  if (sl < nq) {
    qa0 = a.q_p0[q0 + sl];
    qa1 = a.q_p1[q0 + sl];
  }
  const int64_t c_begin = (int64_t)slice * a.per_slice;
  const int64_t c_end = c_begin + a.per_slice < a.N ? c_begin + a.per_slice : a.N;
  for (int64_t c0 = c_begin; c0 < c_end; c0 += SK_STAGE) {    // the same trip count in every thread: barriers inside
    for (int h = 0; h < SK_ROUND; ++h) {
      const int64_t c = c0 + h * SK_GROUPS + grp;
      if (c >= c_end) break;
      int64_t b, e;
      sk_range(a.colptr, c, a.nnz, b, e);
      double acc[TQ];
#pragma unroll
      for (int j = 0; j < TQ; ++j) acc[j] = 0.0;
      sk_chain<TQ, MANH>(a, dense, G, b, e, sl, acc);
      double S = 0.0;
#pragma unroll
      for (int j = 0; j < TQ; ++j) {
        acc[j] = sk_tree(acc[j]);
        if (j == sl) S = acc[j];
      }
      if (sl < nq) {
        const int64_t q = q0 + sl;
        float df = 0.0f;
        if (!SELF || c != q) df = (float)(sk_distance(a.metric, (double)a.G, S, qa0, qa1, a.p0[c], a.p1[c]) + 0.0);
        const u64 key = ((u64)sk_sortable(df) << 32) | (u64)(uint32_t)c;
        if (key < lists[sl * k + k - 1]) {
          const int pos = atomicAdd(&scnt[sl], 1);            // at most one hand-over per candidate and query: pos < SK_STAGE
          stage[sl * SK_STAGE + pos] = key;
        }
      }
    }
    __syncthreads();
    if (wave < nq) {                                          // wave j takes the survivors into query j's list
      const int n = scnt[wave];
      for (int i = 0; i < n; ++i) sk_insert(lists + wave * k, k, stage[wave * SK_STAGE + i], lane);
      if (lane == 0) scnt[wave] = 0;
    }
    __syncthreads();
  }
  if (wave < nq) {
    u64* out = a.part + (((q0 - a.q_begin) + wave) * a.slices + slice) * (int64_t)k;
    for (int p = lane; p < k; p += 64) out[p] = lists[wave * k + p];
  }
}

// ---------------------------------------------------------------- merge
__global__ __launch_bounds__(SK_MERGE_THREADS) void k_sk_merge(const u64* __restrict__ part, int64_t n_q, int slices, int k,
                                                               int32_t* __restrict__ idx, double* __restrict__ dist,
                                                               float* __restrict__ dist32, int64_t ld) {
  __shared__ u64 s_list[SK_MERGE_THREADS / 64][GFICF_KNN_MAX_K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * (SK_MERGE_THREADS / 64) + wave;
  if (q >= n_q) return;                                       // whole waves: no barrier follows
  u64* list = s_list[wave];
  const u64* src = part + q * slices * (int64_t)k;
  for (int p = lane; p < k; p += 64) list[p] = src[p];
  GFICF_WAVE_SYNC();
  for (int s = 1; s < slices; ++s)
    for (int i = 0; i < k; ++i) {
      const u64 x = src[(int64_t)s * k + i];
      if (x >= list[k - 1]) break;                            // a slice's list ascends: nothing further of it fits
      sk_insert(list, k, x, lane);
    }
  for (int p = lane; p < k; p += 64) {
    const u64 key = list[p];
    idx[q + (int64_t)p * ld] = (int32_t)(uint32_t)(key & 0xFFFFFFFFull) + 1;
    const float d = sk_unsortable((uint32_t)(key >> 32));     // the key holds the f32: both tables are exact
    if (dist) dist[q + (int64_t)p * ld] = (double)d;
    if (dist32) dist32[q + (int64_t)p * ld] = d;
  }
}

size_t sk_tile_lds(int64_t G, int tq, int k) {
  return (((size_t)G * tq * sizeof(float) + 15) & ~(size_t)15) + (size_t)tq * (size_t)(k + SK_STAGE) * sizeof(u64) + (size_t)tq * sizeof(int);
}

template <int TQ, bool MANH, bool SELF>
int sk_launch(gficf_ctx* ctx, const SkArgs& a, int64_t tiles) {
  // (per device, and cheap: asked at every launch)
  GFICF_HIP_CHECK(hipFuncSetAttribute((const void*)k_sk_tiles<TQ, MANH, SELF>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64));
  hipLaunchKernelGGL((k_sk_tiles<TQ, MANH, SELF>), dim3((unsigned)tiles, (unsigned)a.slices), dim3(SK_THREADS), sk_tile_lds(a.G, TQ, a.k), ctx->stream, a);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

template <bool MANH, bool SELF>
int sk_launch_tq(gficf_ctx* ctx, const SkArgs& a, int tq, int64_t tiles) {
  switch (tq) {
    case 8: return sk_launch<8, MANH, SELF>(ctx, a, tiles);
    case 4: return sk_launch<4, MANH, SELF>(ctx, a, tiles);
    case 2: return sk_launch<2, MANH, SELF>(ctx, a, tiles);
    default: return sk_launch<1, MANH, SELF>(ctx, a, tiles);
  }
}


}  // namespace
