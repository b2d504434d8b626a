// markers.hip — marker genes: the one-vs-rest Mann-Whitney U test of findClusterMarkers() (reference R/deGenes.R:15-60,
// src/rcpp_parallel_mann_whitney.cpp, src/mann_whitney.cpp) for every cluster at once.  Built into libgficf_markers.so, which
// links libgficf_hip.so and uses its context, pool, scan, radix sort and error plumbing (include/gficf_markers.h).
//
// The ranks of a gene's N values do not depend on the split into "cluster" and "rest", only the rank sums per cluster do, so
// every gene is sorted once for all C clusters.  Only the stored non-zeros are sorted; every zero (implicit, stored, -0.0) falls
// into one tie group whose rank follows from counts.  Launches:
//   k_mk_labels     cluster sizes, labels outside [0, C) flagged
//   (transpose)     gene-major view of the CSC input (gficf_csc_transpose_device), cells ascending within a gene
//   k_mk_gene_of    gene of every entry
//   (addon_sort.h)  k_sort_keys: order-preserving 64-bit key of every value (-0.0 -> +0.0; NaN / Inf flagged); 3 radix sorts,
//                   stable LSD by the key's low 32 bits, its high 32 bits, then the gene (k_sort_next between them): (gene,
//                   value) order
//   k_mk_heads      sorted keys and cluster ids gathered, tie-group heads marked; (scan) -> group numbers
//   k_mk_bounds     first and one-past-last sorted position of every tie group
//   k_mk_walk       one workgroup per gene: 2 * rank, count and 128-bit fixed-point value sum per cluster (LDS while
//                   C <= MK_LDS_MAX_C, global memory beyond), t^3 - t per tie group, the gene's counts
//   k_mk_epilogue   p and log2FC of every (gene, cluster), column-major G x C
// Every accumulation is integer, so the result does not depend on the order of the additions: two calls give the same
// bits, and so does any permutation of the cells together with their labels.
#include <cmath>
#include <vector>

#include "addon_sort.h"
#include "addon_status.h"
#include "common.h"
#include "gficf_markers.h"

namespace {

typedef unsigned long long u64;

constexpr int MK_LDS_MAX_C = 2048;        // 32 B of LDS per cluster: 64 KiB at most per workgroup
constexpr int64_t MK_MAX_N = 2097151;     // Z^3 - Z (and so T) fits int64 for every tie group of up to N cells
constexpr uint32_t MK_ST_LABEL = 1u;      // a label outside [0, C)
constexpr uint32_t MK_ST_EMPTY = 2u;      // a cluster without cells
constexpr uint32_t MK_ST_VALUE = 4u;      // a NaN or infinite value
constexpr int MK_FIXED_MIN_K = 64;        // below this scale a value's truncation can exceed 2^-64: the gene's sums go to f64 instead

struct MkGene {                           // per-gene results of the walk
  int64_t neg, pos;                       // stored entries < 0 and > 0
  int64_t t3;                             // sum of t^3 - t over the non-zero tie groups
  int64_t ndist;                          // distinct non-zero values
  u64 s_lo, s_hi;                         // sum of all values, 128-bit fixed point, scale 2^k
  int32_t k, f64;                         // f64: k < MK_FIXED_MIN_K, the accumulators hold f64 sums (cluster in lo, rest in hi)
};

// the value of a key of gficf_f64_key (whose -0.0 ties with +0.0, as the reference's < and != have it)
__device__ inline double mk_value(u64 key) {
  return __longlong_as_double((long long)((key >> 63) ? (key & ~(1ull << 63)) : ~key));
}

// v * 2^k as a two's-complement 128-bit integer, truncated toward -inf below 2^0 (|v| * 2^k < 2^126 by the choice of k)
__device__ inline __int128 mk_fixed(double v, int k) {
  if (v == 0.0) return 0;
  int e = 0;
  const double m = frexp(v, &e);                           // v = m * 2^e, 0.5 <= |m| < 1
  const long long M = (long long)ldexp(m, 53);             // exact
  const int sh = e - 53 + k;
  if (sh >= 0) return (__int128)M << sh;
  if (sh <= -64) return M < 0 ? -1 : 0;
  return (__int128)(M >> (-sh));
}

__device__ inline double mk_fixed_to_double(u64 lo, u64 hi, int k) {
  return ldexp((double)(long long)hi * 18446744073709551616.0 + (double)lo, -k);
}

// exact 128-bit add into (lo, hi) by atomics: every add's carry out of lo is counted once, whatever the order
__device__ inline void mk_add128(u64* lo, u64* hi, __int128 f) {
  const u64 flo = (u64)f;
  u64 fhi = (u64)((unsigned __int128)f >> 64);
  const u64 old = atomicAdd(lo, flo);
  if (old + flo < old) fhi += 1ull;
  if (fhi) atomicAdd(hi, fhi);
}

__global__ __launch_bounds__(256) void k_mk_labels(int64_t N, const int32_t* __restrict__ cluster, int32_t C, unsigned long long* __restrict__ ncl,
                                                   uint32_t* __restrict__ status) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < N; c += (int64_t)gridDim.x * 256) {
    const int32_t cl = cluster[c];
    if (cl < 0 || cl >= C) { atomicOr(status, MK_ST_LABEL); continue; }
    atomicAdd(&ncl[cl], 1ull);
  }
}

// one wave per gene: gene[p] = g over the gene's range of the gene-major arrays
__global__ __launch_bounds__(256) void k_mk_gene_of(int64_t G, int64_t nnz, const int64_t* __restrict__ tptr, uint32_t* __restrict__ gene) {
  const int lane = threadIdx.x & 63;
  for (int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6; g < G; g += ((int64_t)gridDim.x * 256) >> 6)
    for (int64_t p = tptr[g] + lane; p < tptr[g + 1] && p < nnz; p += 64) gene[p] = (uint32_t)g;
}

// sorted keys and cluster ids; head[i] = 1 where a tie group (of one gene) starts; head[nnz] = 0
__global__ __launch_bounds__(256) void k_mk_heads(int64_t nnz, int64_t N, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ gene_s,
                                                  const u64* __restrict__ key, const int32_t* __restrict__ tidx, const int32_t* __restrict__ cluster,
                                                  u64* __restrict__ ks, uint32_t* __restrict__ cls, int64_t* __restrict__ head) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= nnz; i += (int64_t)gridDim.x * 256) {
    if (i == nnz) { head[i] = 0; continue; }
    const uint32_t p = perm[i];
    const u64 k = key[p];
    ks[i] = k;
    const int32_t cell = tidx[p];
    cls[i] = cell >= 0 && cell < N ? (uint32_t)cluster[cell] : 0u;     // (entries a malformed CSC left unplaced: BAD_CSC is raised)
    head[i] = (i == 0 || gene_s[i] != gene_s[i - 1] || key[perm[i - 1]] != k) ? 1 : 0;
  }
}

// e[] = exclusive scan of the heads: sorted position i belongs to group e[i + 1] - 1
__global__ __launch_bounds__(256) void k_mk_bounds(int64_t nnz, const int64_t* __restrict__ e, uint32_t* __restrict__ gstart, uint32_t* __restrict__ gend) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * 256) {
    const int64_t g1 = e[i + 1];
    if (g1 - e[i] == 1) gstart[g1 - 1] = (uint32_t)i;
    if (i == nnz - 1 || e[i + 2] - g1 == 1) gend[g1 - 1] = (uint32_t)(i + 1);
  }
}

// accumulators of gene g, C wide: r2 (sum of 2 * rank over the cluster's non-zero entries), cnt (its non-zero entries),
// s_lo / s_hi (its value sum, 128-bit fixed point); LDS: the workgroup's own copy, written out at the end; GLOBAL: rows g of
// the G x C arrays themselves (zeroed by the caller).
// A gene whose largest |v| puts the scale k below MK_FIXED_MIN_K (|v| >= 2^(61 - nb): beyond 2^50 at 2000 cells, 2^39 at 2^21)
// would lose its small values to the truncation.  Its value sums are taken in f64 instead: thread 0 adds the gene's entries in
// sorted order (canonical: tied entries hold equal values) into lo[c], then writes each cluster's rest into hi[c] as the sum over
// the clusters before it plus the sum over those after it (never total - cluster, which cancels when the cluster holds the huge
// value).  Sequential, so only for such genes; every other gene keeps the integer path and its bits.
template <bool LDS>
__global__ __launch_bounds__(256) void k_mk_walk(int64_t G, int64_t N, int nb, int64_t nnz, int32_t C, const int64_t* __restrict__ tptr, const u64* __restrict__ ks,
                                                 const uint32_t* __restrict__ cls, const int64_t* __restrict__ e, const uint32_t* __restrict__ gstart,
                                                 const uint32_t* __restrict__ gend, u64* __restrict__ a_r2, u64* __restrict__ a_cnt,
                                                 u64* __restrict__ a_lo, u64* __restrict__ a_hi, MkGene* __restrict__ gst) {
  extern __shared__ u64 s_acc[];                           // LDS: 4 x C
  __shared__ int64_t s_red[4];
  __shared__ u64 s_tot[2];
  const int lane = threadIdx.x & 63;
  for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
    u64 *r2, *cnt, *lo, *hi;
    if (LDS) {
      r2 = s_acc; cnt = s_acc + C; lo = s_acc + 2 * (int64_t)C; hi = s_acc + 3 * (int64_t)C;
      for (int t = threadIdx.x; t < 4 * C; t += 256) s_acc[t] = 0ull;
    } else {
      r2 = a_r2 + g * C; cnt = a_cnt + g * C; lo = a_lo + g * C; hi = a_hi + g * C;
    }
    if (threadIdx.x < 4) s_red[threadIdx.x] = 0;
    if (threadIdx.x < 2) s_tot[threadIdx.x] = 0ull;
    __syncthreads();
    const int64_t b = tptr[g], end = tptr[g + 1] < nnz ? tptr[g + 1] : nnz, nnz_g = end > b ? end - b : 0;
    int k = 0;
    bool f64 = false;
    if (nnz_g > 0) {
      const double mx = fmax(fabs(mk_value(ks[b])), fabs(mk_value(ks[end - 1])));
      if (mx > 0.0) k = 125 - ilogb(mx) - nb;        // N < 2^nb: N * max|v| * 2^k < 2^126
      f64 = mx > 0.0 && k < MK_FIXED_MIN_K;
    }
    int64_t neg = 0, pos = 0, t3 = 0, nd = 0;
    __int128 tot = 0;
    for (int64_t i = b + threadIdx.x; i < end; i += 256) {
      const double v = mk_value(ks[i]);
      if (v == 0.0) continue;                              // stored zeros join the zero group (counted from the sizes)
      const int64_t grp = e[i + 1] - 1;
      const int64_t s = gstart[grp], t = (int64_t)gend[grp] - s;
      const int64_t pos0 = s - b + (v > 0.0 ? N - nnz_g : 0);
      const uint32_t c = cls[i];
      if (c >= (uint32_t)C) continue;                      // a label outside [0, C): raised by k_mk_labels
      atomicAdd(&r2[c], (u64)(2 * pos0 + t + 1));
      atomicAdd(&cnt[c], 1ull);
      if (!f64) {
        const __int128 f = mk_fixed(v, k);
        mk_add128(&lo[c], &hi[c], f);
        tot += f;
      }
      if (v < 0.0) ++neg; else ++pos;
      if (i == s) { t3 += t * t * t - t; ++nd; }
    }
    neg = gficf_wave_sum(neg); pos = gficf_wave_sum(pos); t3 = gficf_wave_sum(t3); nd = gficf_wave_sum(nd);
    u64 tlo = (u64)tot, thi = (u64)((unsigned __int128)tot >> 64);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const u64 olo = __shfl_xor(tlo, d), ohi = __shfl_xor(thi, d);
      const u64 nlo = tlo + olo;
      thi = thi + ohi + (nlo < tlo ? 1ull : 0ull);
      tlo = nlo;
    }
    if (lane == 0) {
      atomicAdd((unsigned long long*)&s_red[0], (u64)neg); atomicAdd((unsigned long long*)&s_red[1], (u64)pos);
      atomicAdd((unsigned long long*)&s_red[2], (u64)t3); atomicAdd((unsigned long long*)&s_red[3], (u64)nd);
      mk_add128(&s_tot[0], &s_tot[1], (__int128)(((unsigned __int128)thi << 64) | tlo));
    }
    __syncthreads();
    if (f64) {
      if (threadIdx.x == 0) {
        for (int64_t i0 = b; i0 < end; i0 += 8) {          // eight entries' loads in flight
          u64 kk[8];
          uint32_t cc[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) { const int64_t i = i0 + j < end ? i0 + j : end - 1; kk[j] = ks[i]; cc[j] = cls[i]; }
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const double v = mk_value(kk[j]);
            if (i0 + j < end && v != 0.0 && cc[j] < (uint32_t)C) lo[cc[j]] = (u64)__double_as_longlong(__longlong_as_double((long long)lo[cc[j]]) + v);
          }
        }
        double run = 0.0;
        for (int c = 0; c < C; ++c) { hi[c] = (u64)__double_as_longlong(run); run += __longlong_as_double((long long)lo[c]); }
        run = 0.0;
        for (int c = C - 1; c >= 0; --c) {
          hi[c] = (u64)__double_as_longlong(__longlong_as_double((long long)hi[c]) + run);
          run += __longlong_as_double((long long)lo[c]);
        }
      }
      __syncthreads();
    }
    if (LDS)
      for (int t = threadIdx.x; t < C; t += 256) {
        a_r2[g * C + t] = r2[t]; a_cnt[g * C + t] = cnt[t]; a_lo[g * C + t] = lo[t]; a_hi[g * C + t] = hi[t];
      }
    if (threadIdx.x == 0) {
      MkGene o;
      o.neg = s_red[0]; o.pos = s_red[1]; o.t3 = s_red[2]; o.ndist = s_red[3];
      o.s_lo = s_tot[0]; o.s_hi = s_tot[1]; o.k = k; o.f64 = f64 ? 1 : 0;
      gst[g] = o;
    }
    __syncthreads();                                       // LDS reused by the next gene
  }
}

// The reference's arithmetic (src/rcpp_parallel_mann_whitney.cpp:62-100, src/mann_whitney.cpp getSigma / getPvalue), z bit for bit:
// no contraction of the sigma expression into fused multiply-adds.
__global__ __launch_bounds__(256) void k_mk_epilogue(int64_t G, int64_t N, int32_t C, const u64* __restrict__ ncl, const u64* __restrict__ a_r2,
                                                     const u64* __restrict__ a_cnt, const u64* __restrict__ a_lo, const u64* __restrict__ a_hi,
                                                     const MkGene* __restrict__ gst, double* __restrict__ p_out, double* __restrict__ lfc_out,
                                                     uint32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int64_t total = G * (int64_t)C;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int64_t g = q % G, c = q / G;                    // g fastest: the stores of a wave are contiguous
    const int64_t n1 = (int64_t)ncl[c], n2 = N - n1;
    if (n1 == 0) {
      if (g == 0) atomicOr(status, MK_ST_EMPTY);
      p_out[q] = NAN; lfc_out[q] = NAN;
      continue;
    }
    const MkGene s = gst[g];
    const int64_t a = g * C + c;
    const int64_t Z = N - s.neg - s.pos;                   // the zero group
    const int64_t r2c = (int64_t)a_r2[a] + (n1 - (int64_t)a_cnt[a]) * (2 * s.neg + Z + 1);
    const int64_t u1 = r2c - n1 * (n1 + 1), u2 = (N * (N + 1) - r2c) - n2 * (n2 + 1);     // 2 * U1, 2 * U2
    double p = 1.0;
    if (s.ndist + (Z > 0 ? 1 : 0) > 1) {
      const int64_t mu = (n1 * n2) / 2;                    // size_t division: floored
      double z = (double)((u1 < u2 ? u1 : u2) - 2 * mu) * 0.5;
      z = z < 0 ? z + 0.5 : z - 0.5;
      const int64_t T = s.t3 + (Z * Z * Z - Z);
      const double d1 = (double)n1, d2 = (double)n2;
      const double sig = sqrt((d1 * d2 / 12) * ((d1 + d2 + 1) - (double)T / ((d1 + d2) * (d1 + d2 - 1))));
      z = z / sig;
      p = erfc(fabs(z) / 1.4142135623730951);
    }
    // log2(avg(v1 + 1) / avg(v2 + 1)); the rest's sum = the gene's total - the cluster's, exact in fixed point (f64 genes: both
    // sums as the walk left them)
    const u64 clo = a_lo[a], chi = a_hi[a];
    const u64 rlo = s.s_lo - clo, rhi = s.s_hi - chi - (s.s_lo < clo ? 1ull : 0ull);
    const double sc = s.f64 ? __longlong_as_double((long long)clo) : mk_fixed_to_double(clo, chi, s.k);
    const double sr = s.f64 ? __longlong_as_double((long long)chi) : mk_fixed_to_double(rlo, rhi, s.k);
    p_out[q] = p;
    lfc_out[q] = log2(((sc + (double)n1) / (double)n1) / ((sr + (double)n2) / (double)n2));
  }
}
// ------------------------------------------------------- the dense two-matrix form: [X | Y] gene-major, cells of X labelled 0, of Y 1
constexpr int MK_DENSE_CHUNK = 256;        // cells a thread walks: count[g][chunk] entries, scanned, then placed in the same order

__device__ inline double mk_dense_at(int64_t G, int64_t n1, const double* X, const double* Y, int64_t g, int64_t j) {
  return j < n1 ? X[g + j * G] : Y[g + (j - n1) * G];
}

template <bool PLACE>
__global__ __launch_bounds__(256) void k_mk_dense(int64_t G, int64_t n1, int64_t n2, const double* __restrict__ X, const double* __restrict__ Y,
                                                  int64_t nch, int64_t* __restrict__ cnt, int32_t* __restrict__ tidx, double* __restrict__ tx) {
  const int64_t N = n1 + n2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < G * nch; q += (int64_t)gridDim.x * 256) {
    const int64_t g = q % G, ch = q / G;                   // g fastest: a wave reads 64 consecutive doubles of one column
    const int64_t j1 = (ch + 1) * MK_DENSE_CHUNK < N ? (ch + 1) * MK_DENSE_CHUNK : N;
    int64_t o = PLACE ? cnt[g * nch + ch] : 0;
    for (int64_t j = ch * MK_DENSE_CHUNK; j < j1; ++j) {
      const double v = mk_dense_at(G, n1, X, Y, g, j);
      if (v != 0.0) {
        if (PLACE) { tidx[o] = (int32_t)j; tx[o] = v; }
        ++o;
      }
    }
    if (!PLACE) cnt[g * nch + ch] = o;
  }
}

__global__ __launch_bounds__(256) void k_mk_dense_ptr(int64_t G, int64_t nch, int64_t n1, int64_t N, const int64_t* __restrict__ cnt,
                                                      int64_t* __restrict__ tptr, int32_t* __restrict__ cluster) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= G || i < N; i += (int64_t)gridDim.x * 256) {
    if (i <= G) tptr[i] = cnt[i * nch];
    if (i < N) cluster[i] = i < n1 ? 0 : 1;
  }
}

// ------------------------------------------------------- workspace
struct MkWs {
  uint32_t* status;
  u64* ncl;
  void* tr_ws;
  size_t tr_bytes;
  int64_t* tptr;
  int32_t* tidx;
  double* tx;
  gficf_sort_bufs sort;
  uint32_t *gene, *cls, *gstart, *gend;
  MkGene* gst;
  u64 *r2, *cnt, *lo, *hi;
};

static size_t mk_carve(char* base, int64_t G, int64_t N, int64_t nnz, int64_t C, MkWs& w) {
  gficf_carver cv;
  cv.base = base;
  const size_t n1 = (size_t)(nnz > 0 ? nnz : 1), gc = (size_t)G * (size_t)C;
  w.status = cv.take<uint32_t>(1);
  w.ncl = cv.take<u64>((size_t)C);
  w.tr_bytes = gficf_csc_transpose_workspace_bytes(G, N);
  w.tr_ws = cv.take<char>(w.tr_bytes);
  w.tptr = cv.take<int64_t>((size_t)G + 1);
  w.tidx = cv.take<int32_t>(n1);
  w.tx = cv.take<double>(n1);
  w.sort.take(cv, n1, n1, {gficf_bit_width(G)});
  w.gene = cv.take<uint32_t>(n1);
  w.cls = cv.take<uint32_t>(n1);
  w.gstart = cv.take<uint32_t>(n1);
  w.gend = cv.take<uint32_t>(n1);
  w.gst = cv.take<MkGene>((size_t)G);
  w.r2 = cv.take<u64>(gc);
  w.cnt = cv.take<u64>(gc);
  w.lo = cv.take<u64>(gc);
  w.hi = cv.take<u64>(gc);
  return cv.total();
}

static int mk_check_sizes(int64_t G, int64_t N, int64_t nnz, int64_t C) {
  if (G < 0 || N < 0 || nnz < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative size");
  if (C < 2 || C > INT32_MAX) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "C = %lld: a one-vs-rest test needs at least 2 clusters", (long long)C);
  if (N < C) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "%lld cells cannot fill %lld clusters", (long long)N, (long long)C);
  if (N > MK_MAX_N) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than %lld cells (the tie sum T must fit int64)", (long long)MK_MAX_N);
  if (nnz > (int64_t)UINT32_MAX - 1) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^32 - 2 stored entries");
  if (G > (int64_t)UINT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^32 - 1 genes");
  return GFICF_OK;
}

// from the gene-major view (w.tptr / w.tidx / w.tx, nnz entries) and the cluster sizes (w.ncl) on: sort, walk, epilogue
static int mk_core(gficf_ctx* ctx, const MkWs& w, int64_t G, int64_t N, int64_t nnz, const int32_t* d_cluster, int32_t C, double* d_p,
                   double* d_lfc) {
  hipStream_t st = ctx->stream;
  const gficf_sort_bufs& s = w.sort;
  if (nnz > 0) {
    hipLaunchKernelGGL(k_mk_gene_of, dim3(gficf_grid_1d(G * 64)), dim3(256), 0, st, G, nnz, (const int64_t*)w.tptr, w.gene);
    GFICF_HIP_CHECK(hipGetLastError());
    int rc = gficf_sort_f64(ctx, s, nnz, {w.tx, 0, nullptr, w.status, MK_ST_VALUE, nullptr, w.gene, 0u, gficf_bit_width(G)});   // (gene, value) order
    if (rc) return rc;
    int64_t* const head = (int64_t*)s.kv1;
    hipLaunchKernelGGL(k_mk_heads, dim3(gficf_grid_1d(nnz + 1)), dim3(256), 0, st, nnz, N, (const uint32_t*)s.oval, (const uint32_t*)s.okey, (const u64*)s.key,
                       (const int32_t*)w.tidx, d_cluster, s.kv0, w.cls, head);
    GFICF_HIP_CHECK(hipGetLastError());
    rc = gficf_exclusive_scan_i64(ctx, head, nnz + 1);
    if (rc) return rc;
    hipLaunchKernelGGL(k_mk_bounds, dim3(gficf_grid_1d(nnz)), dim3(256), 0, st, nnz, (const int64_t*)head, w.gstart, w.gend);
    GFICF_HIP_CHECK(hipGetLastError());
  }
  const unsigned wg = (unsigned)(G < (1 << 20) ? (G > 0 ? G : 1) : (1 << 20));
  if (C <= MK_LDS_MAX_C) {
    hipLaunchKernelGGL(k_mk_walk<true>, dim3(wg), dim3(256), (size_t)C * 4 * sizeof(u64), st, G, N, gficf_bit_width(N), nnz, C, (const int64_t*)w.tptr, (const u64*)s.kv0,
                       (const uint32_t*)w.cls, (const int64_t*)s.kv1, (const uint32_t*)w.gstart, (const uint32_t*)w.gend, w.r2, w.cnt, w.lo, w.hi, w.gst);
  } else {
    const size_t gc = (size_t)G * (size_t)C * sizeof(u64);
    GFICF_HIP_CHECK(hipMemsetAsync(w.r2, 0, gc, st));
    GFICF_HIP_CHECK(hipMemsetAsync(w.cnt, 0, gc, st));
    GFICF_HIP_CHECK(hipMemsetAsync(w.lo, 0, gc, st));
    GFICF_HIP_CHECK(hipMemsetAsync(w.hi, 0, gc, st));
    hipLaunchKernelGGL(k_mk_walk<false>, dim3(wg), dim3(256), 0, st, G, N, gficf_bit_width(N), nnz, C, (const int64_t*)w.tptr, (const u64*)s.kv0, (const uint32_t*)w.cls,
                       (const int64_t*)s.kv1, (const uint32_t*)w.gstart, (const uint32_t*)w.gend, w.r2, w.cnt, w.lo, w.hi, w.gst);
  }
  GFICF_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_mk_epilogue, dim3(gficf_grid_1d(G * C)), dim3(256), 0, st, G, N, C, (const u64*)w.ncl, (const u64*)w.r2, (const u64*)w.cnt,
                     (const u64*)w.lo, (const u64*)w.hi, (const MkGene*)w.gst, d_p, d_lfc, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// the labels on the host: in [0, C), every cluster non-empty
static int mk_check_labels(const int32_t* cluster, int64_t N, int32_t C) {
  std::vector<int64_t> n((size_t)C, 0);
  for (int64_t c = 0; c < N; ++c) {
    const int32_t l = cluster[c];
    if (l < 0 || l >= C) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "cluster[%lld] = %d is outside [0, %d)", (long long)c, l, C);
    ++n[(size_t)l];
  }
  for (int32_t l = 0; l < C; ++l)
    if (!n[(size_t)l]) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "cluster %d has no cells", l);
  return GFICF_OK;
}

}  // namespace

extern "C" {

int gficf_markers_abi_version(void) { return GFICF_MARKERS_ABI_VERSION; }

size_t gficf_cluster_markers_workspace_bytes(int64_t G, int64_t N, int64_t nnz, int32_t C) {
  if (G < 0 || N < 0 || nnz < 0 || C < 0) return 0;
  MkWs w;
  return mk_carve(nullptr, G, N, nnz, C, w);
}

int gficf_cluster_markers_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int64_t nnz,
                                 const int32_t* d_cluster, int32_t C, void* ws, size_t ws_bytes, double* d_p, double* d_lfc) {
  GFICF_CTX_ENTER(ctx);
  int rc = mk_check_sizes(G, N, nnz, C);
  if (rc) return rc;
  if (!d_colptr || !d_cluster || !ws || (G > 0 && (!d_p || !d_lfc)) || (nnz > 0 && (!d_rowidx || !d_x)))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  MkWs w;
  rc = gficf_addon_carve(ws, ws_bytes, [&](char* base) { return mk_carve(base, G, N, nnz, C, w); });
  if (rc) return rc;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), ctx->stream));
  GFICF_HIP_CHECK(hipMemsetAsync(w.ncl, 0, sizeof(u64) * (size_t)C, ctx->stream));
  hipLaunchKernelGGL(k_mk_labels, dim3(gficf_grid_1d(N)), dim3(256), 0, ctx->stream, N, d_cluster, C, w.ncl, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  if (G == 0) return GFICF_OK;
  rc = gficf_csc_transpose_device(ctx, G, N, d_colptr, d_rowidx, d_x, nnz, w.tptr, w.tidx, w.tx, w.tr_ws, w.tr_bytes);
  if (rc) return rc;
  return mk_core(ctx, w, G, N, nnz, d_cluster, C, d_p, d_lfc);
}

int gficf_cluster_markers_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  const int rc = gficf_addon_read_status(ctx, ws, &st);
  if (rc) return rc;
  if (st & MK_ST_LABEL) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a cluster label outside [0, C)");
  if (st & MK_ST_EMPTY) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a cluster without cells");
  if (st & MK_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "the expression matrix holds a NaN or an infinite value");
  return GFICF_OK;
}

int gficf_cluster_markers_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x,
                               const int32_t* cluster, int32_t C, double* p, double* lfc) {
  GFICF_CTX_ENTER(ctx);
  if (G < 0 || N < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative size");
  if (!colptr || !cluster || (G > 0 && (!p || !lfc))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> cp;
  int64_t nnz = 0;
  int rc = gficf_host_colptr(colptr, colptr_is_i64, N, "colptr", cp, &nnz);
  if (rc) return rc;
  rc = mk_check_sizes(G, N, nnz, C);
  if (rc) return rc;
  if (nnz > 0 && (!rowidx || !x)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  rc = mk_check_labels(cluster, N, C);
  if (rc) return rc;
  const size_t nsz = (size_t)(nnz > 0 ? nnz : 1), gc = (size_t)G * (size_t)C;
  const size_t wsb = gficf_cluster_markers_workspace_bytes(G, N, nnz, C);
  gficf_host_io io{ctx, "gficf_cluster_markers_host"};
  gficf_carver cv;
  int64_t* d_cp; int32_t *d_ri, *d_cl; double *d_x, *d_p, *d_l; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_cp = cv.take<int64_t>((size_t)N + 1); d_ri = cv.take<int32_t>(nsz); d_x = cv.take<double>(nsz);
    d_cl = cv.take<int32_t>((size_t)N); d_p = cv.take<double>(gc); d_l = cv.take<double>(gc);
    d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_cp, cp.data(), sizeof(int64_t) * cp.size());
  io.up(d_ri, rowidx, sizeof(int32_t) * (size_t)nnz);
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  io.up(d_cl, cluster, sizeof(int32_t) * (size_t)N);
  if (io.ok()) {
    rc = gficf_cluster_markers_device(ctx, G, N, d_cp, d_ri, d_x, nnz, d_cl, C, d_ws, wsb, d_p, d_l);
    if (!rc) {
      io.down(p, d_p, sizeof(double) * gc);
      io.down(lfc, d_l, sizeof(double) * gc);
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_cluster_markers_sync(ctx, d_ws);
}

int gficf_cluster_markers_dense_host(gficf_ctx* ctx, int64_t G, int64_t n1, const double* X, int64_t n2, const double* Y, double* out) {
  GFICF_CTX_ENTER(ctx);
  if (G < 0 || n1 < 0 || n2 < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative size");
  if (n1 < 1 || n2 < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "both samples need at least one cell (n1 = %lld, n2 = %lld)", (long long)n1, (long long)n2);
  const int64_t N = n1 + n2;
  int rc = mk_check_sizes(G, N, 0, 2);
  if (rc) return rc;
  if (G == 0) return GFICF_OK;
  if (!X || !Y || !out) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  if ((double)G * (double)N > (double)UINT32_MAX - 2) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^32 - 2 entries");
  hipStream_t st = ctx->stream;
  const int64_t nch = gficf_ceil_div(N, MK_DENSE_CHUNK);
  gficf_host_io io{ctx, "gficf_cluster_markers_dense_host"};
  gficf_carver cv;                                         // STAGE0: the inputs, the count matrix and the results; STAGE1: the workspace
  double *dX, *dY, *dp, *dl; int64_t* cnt; int32_t* dcl;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    dX = cv.take<double>((size_t)(G * n1)); dY = cv.take<double>((size_t)(G * n2));
    cnt = cv.take<int64_t>((size_t)(G * nch + 1)); dcl = cv.take<int32_t>((size_t)N);
    dp = cv.take<double>((size_t)G * 2); dl = cv.take<double>((size_t)G * 2);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(dX, X, sizeof(double) * (size_t)(G * n1));
  io.up(dY, Y, sizeof(double) * (size_t)(G * n2));
  if (!io.ok()) return io.drain(GFICF_OK);
  GFICF_HIP_CHECK(hipMemsetAsync(cnt + G * nch, 0, sizeof(int64_t), st));
  hipLaunchKernelGGL(k_mk_dense<false>, dim3(gficf_grid_1d(G * nch)), dim3(256), 0, st, G, n1, n2, dX, dY, nch, cnt, (int32_t*)nullptr, (double*)nullptr);
  GFICF_HIP_CHECK(hipGetLastError());
  rc = gficf_exclusive_scan_i64(ctx, cnt, G * nch + 1);
  if (rc) return rc;
  int64_t nnz = 0;
  GFICF_HIP_CHECK(hipMemcpyAsync(&nnz, cnt + G * nch, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  GFICF_HIP_CHECK(hipStreamSynchronize(st));
  const size_t wsb = gficf_cluster_markers_workspace_bytes(G, N, nnz, 2);
  void* wsp = nullptr;
  GFICF_HIP_CHECK(gficf_pool_get(ctx, GFICF_SLOT_STAGE1, wsb, &wsp));
  MkWs w;
  mk_carve((char*)wsp, G, N, nnz, 2, w);
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.ncl, 0, sizeof(u64) * 2, st));
  hipLaunchKernelGGL(k_mk_dense<true>, dim3(gficf_grid_1d(G * nch)), dim3(256), 0, st, G, n1, n2, dX, dY, nch, cnt, w.tidx, w.tx);
  hipLaunchKernelGGL(k_mk_dense_ptr, dim3(gficf_grid_1d((G > N ? G : N) + 1)), dim3(256), 0, st, G, nch, n1, N, (const int64_t*)cnt, w.tptr, dcl);
  hipLaunchKernelGGL(k_mk_labels, dim3(gficf_grid_1d(N)), dim3(256), 0, st, N, (const int32_t*)dcl, 2, w.ncl, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  rc = mk_core(ctx, w, G, N, nnz, dcl, 2, dp, dl);
  if (!rc) {                                     // out = [p, log2FC] of the first sample (cluster 0): column 0 of each G x 2 result
    io.down(out, dp, sizeof(double) * (size_t)G);
    io.down(out + G, dl, sizeof(double) * (size_t)G);
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_cluster_markers_sync(ctx, w.status);
}

}  // extern "C"
