// gsva.hip — GSVA scores of every cell within its cluster and the two-group sums of the limma contrasts: the method = "GSVA"
// branch of runGSEA() (reference R/pathwayAnalisys.R:97-138) for all clusters and pathways at once.  Built into
// libgficf_gsva.so, which links libgficf_hip.so and uses its context, pool, radix sort and error plumbing
// (include/gficf_gsva.h states the contract).
//
// Nothing is densified.  The zeros of a gene within a cluster are one group with one density d0, so the order of a cell's
// genes is the cluster's order of the d0 with the cell's stored genes taken out and put back at the places of their own
// densities: the position of a gene is its rank among the d0 keys, minus the number of the cell's stored genes whose d0 key
// precedes it, plus the number whose real key precedes it -- two searches in two sorted lists of the cell's stored genes held
// in LDS.  A set of positions is a bit mask in LDS and its running sums a popcount scan, as in gsea.hip.
// Launches, all on the context's stream:
//   k_gv_count       n_c, the cells of every cluster (integer atomics); a cluster id out of range is flagged
//   k_gv_density     one workgroup per (gene, cluster) segment and range of GFICF_GSVA_JSPLIT entries j: mean, sd, kept, d0,
//                    and d_j of its j, the segment's x_i staged through LDS in tiles of 256, one x_j per lane
//   k_gv_gc          G_c, the kept genes of every cluster
//   (addon_sort.h)   k_sort_keys: descending 64-bit key of every d0 (a gene that is not kept sorts last); 3 radix sorts, stable
//                    LSD by the key's low 32 bits, its high 32 bits, then the cluster (k_sort_next between them): (cluster,
//                    d0 desc, row) order
//   k_gv_rank        the rank of every gene in its cluster's order, and the keys in that order
//   k_gv_sizes       one workgroup per pathway: members checked (range, repeats), m_pc and tested for every cluster
//   k_gv_walk        one workgroup per cell: its stored kept genes into the two LDS lists (bitonic sort), their positions,
//                    then every tested pathway: member positions into the mask, scan, ES
//   k_gv_sums        one thread per (pathway, cluster): sum and sum of squares over the cluster's cells in ascending order
#include <algorithm>
#include <cmath>
#include <vector>

#include "addon_sort.h"
#include "addon_status.h"
#include "common.h"
#include "gficf_gsva.h"

namespace {

typedef unsigned long long u64;

constexpr int GV_MAX_WORDS = GFICF_GSVA_MAX_G / 32;   // the LDS mask: 16 KiB
constexpr uint32_t GV_ST_VALUE = 1u;                  // a NaN or infinite value or density
constexpr uint32_t GV_ST_CLUSTER = 2u;                // a cluster id outside [0, C)
constexpr uint32_t GV_ST_RANGE = 4u;                  // a member outside [0, G)
constexpr uint32_t GV_ST_DUP = 8u;                    // a member repeated within a pathway
constexpr uint32_t GV_ST_GROUP = 16u;                 // a segment with an entry of another cluster, or with more entries than cells
constexpr uint32_t GV_ST_INDEX = 32u;                 // a cell, row or src index out of range, rows of a cell that do not ascend
constexpr uint32_t GV_ST_PTR = 64u;                   // offsets that decrease or leave their array
constexpr double GV_MIN_SD = 1e-10;
constexpr double GV_INV_SQRT2 = 0.7071067811865476;

__global__ __launch_bounds__(256) void k_gv_count(int64_t N, int32_t C, const int32_t* __restrict__ cluster, int32_t* __restrict__ n_c,
                                                  uint32_t* __restrict__ status) {
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < N; j += (int64_t)gridDim.x * 256) {
    const int32_t c = cluster[j];
    if (c < 0 || c >= C) atomicOr(status, GV_ST_CLUSTER);
    else atomicAdd(&n_c[c], 1);
  }
}

// block (s, y): segment s = g * C + c, entries j in [y * JSPLIT, (y + 1) * JSPLIT)
__global__ __launch_bounds__(256) void k_gv_density(int64_t N, int32_t C, const int32_t* __restrict__ cluster, const int32_t* __restrict__ n_c,
                                                    const int64_t* __restrict__ seg_ptr, const int32_t* __restrict__ cell,
                                                    const double* __restrict__ x, int64_t nnz, double* __restrict__ sd, double* __restrict__ d0,
                                                    int32_t* __restrict__ kept, double* __restrict__ dnz, uint32_t* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double s_fold[256];
  __shared__ double s_x[GFICF_GSVA_TILE];
  const int t = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int32_t c = (int32_t)(s % C);
  const int64_t g = s / C, out = (int64_t)c * (int64_t)(gridDim.x / C) + g;   // G x C column-major
  const bool first = blockIdx.y == 0;
  const int64_t beg = seg_ptr[s], end = seg_ptr[s + 1];
  if (beg < 0 || end < beg || end > nnz) {
    if (first && t == 0) { atomicOr(status, GV_ST_PTR); sd[out] = 0.0; d0[out] = 0.0; kept[out] = 0; }
    return;
  }
  const int64_t nz = end - beg, j_beg = (int64_t)blockIdx.y * GFICF_GSVA_JSPLIT;
  if (!first && j_beg >= nz) return;
  const int64_t j_end = j_beg + GFICF_GSVA_JSPLIT < nz ? j_beg + GFICF_GSVA_JSPLIT : nz;
  const int64_t n = n_c[c];
  const double* xs = x + beg;
  if (nz > n) {                                            // an entry per cell at the most
    if (first && t == 0) { atomicOr(status, GV_ST_GROUP); sd[out] = 0.0; d0[out] = 0.0; kept[out] = 0; }
    for (int64_t j = j_beg + t; j < j_end; j += 256) dnz[beg + j] = 0.0;
    return;
  }
  const double dn = (double)n, dz = (double)(n - nz);
  double a = 0.0;
  for (int64_t i = t; i < nz; i += 256) {
    const double v = xs[i];
    if (first) {
      const int32_t ce = cell[beg + i];
      if (ce < 0 || (int64_t)ce >= N) atomicOr(status, GV_ST_INDEX);
      else if (cluster[ce] != c) atomicOr(status, GV_ST_GROUP);
      if (!isfinite(v)) atomicOr(status, GV_ST_VALUE);
    }
    a += v;
  }
  const double mean = gficf_block_sum_f64(a, s_fold) / dn;
  a = 0.0;
  for (int64_t i = t; i < nz; i += 256) {
    const double e = xs[i] - mean;
    a += e * e;
  }
  const double ss = gficf_block_sum_f64(a, s_fold) + dz * (mean * mean);
  const double sdv = n >= 2 ? sqrt(ss / (double)(n - 1)) : 0.0;
  const bool keep = n >= 2 && sdv >= GV_MIN_SD;
  if (!keep) {
    if (first && t == 0) { sd[out] = sdv == sdv ? sdv : 0.0; d0[out] = 0.0; kept[out] = 0; }
    for (int64_t j = j_beg + t; j < j_end; j += 256) dnz[beg + j] = 0.0;
    return;
  }
  const double r = GV_INV_SQRT2 / (sdv / 4.0);
  if (first) {
    double v0 = 0.0;
    if (nz < n) {
      a = 0.0;
      for (int64_t i = t; i < nz; i += 256) a += 0.5 * erfc(xs[i] * r);
      const double L0 = (gficf_block_sum_f64(a, s_fold) + 0.5 * dz) / dn;
      v0 = -log((1.0 - L0) / L0);
    }
    if (t == 0) { sd[out] = sdv; d0[out] = v0; kept[out] = 1; }
  }
  for (int64_t j0 = j_beg; j0 < j_end; j0 += GFICF_GSVA_TILE) {
    const int64_t j = j0 + t;
    const bool mine = j < j_end;
    const double xj = mine ? xs[j] : 0.0;
    double acc = 0.0;
    for (int64_t i0 = 0; i0 < nz; i0 += GFICF_GSVA_TILE) {
      __syncthreads();
      if (i0 + t < nz) s_x[t] = xs[i0 + t];
      __syncthreads();
      const int len = (int)(nz - i0 < GFICF_GSVA_TILE ? nz - i0 : GFICF_GSVA_TILE);
      if (mine)
        for (int i = 0; i < len; ++i) acc += 0.5 * erfc((s_x[i] - xj) * r);
    }
    if (mine) {
      const double L = (acc + dz * (0.5 * erfc(-xj * r))) / dn;
      dnz[beg + j] = -log((1.0 - L) / L);
    }
  }
}

// one workgroup per cluster
__global__ __launch_bounds__(256) void k_gv_gc(int64_t G, const int32_t* __restrict__ kept, int32_t* __restrict__ gc) {
  __shared__ int32_t s_c[4];
  const int t = threadIdx.x;
  const int32_t* col = kept + (int64_t)blockIdx.x * G;
  int32_t cnt = 0;
  for (int64_t g = t; g < G; g += 256) cnt += col[g] != 0 ? 1 : 0;
  cnt = gficf_wave_sum(cnt);
  if ((t & 63) == 0) s_c[t >> 6] = cnt;
  __syncthreads();
  if (t == 0) gc[blockIdx.x] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
}

// sorted position i holds val[i] = c * G + g; cluster c fills [c * G, (c + 1) * G)
__global__ __launch_bounds__(256) void k_gv_rank(int64_t n, uint32_t G, const uint32_t* __restrict__ val, const u64* __restrict__ key,
                                                 int32_t* __restrict__ rank, u64* __restrict__ skey) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t p = val[i];
    if ((int64_t)p < n) {
      rank[p] = (int32_t)(i - (int64_t)(p / G) * G);
      skey[i] = key[p];
    }
  }
}

// one workgroup per pathway: its members checked once, then counted in every cluster
__global__ __launch_bounds__(256) void k_gv_sizes(int32_t G, int32_t C, int64_t P, const int64_t* __restrict__ ptr, int64_t n_members,
                                                  const int32_t* __restrict__ members, const int32_t* __restrict__ kept, const int32_t* __restrict__ n_c,
                                                  const int32_t* __restrict__ gc, int64_t lo, int64_t hi, int32_t* __restrict__ msize,
                                                  int32_t* __restrict__ tested, uint32_t* __restrict__ status) {
  __shared__ uint32_t s_mask[GV_MAX_WORDS];
  __shared__ int32_t s_c[4];
  const int t = threadIdx.x;
  const int64_t p = blockIdx.x, beg = ptr[p], len = ptr[p + 1] - beg;
  if (beg < 0 || len < 0 || beg + len > n_members) {
    if (t == 0) atomicOr(status, GV_ST_PTR);
    for (int c = t; c < C; c += 256) { msize[(int64_t)c * P + p] = 0; tested[(int64_t)c * P + p] = 0; }
    return;
  }
  const int W = (G + 31) >> 5;
  for (int w = t; w < W; w += 256) s_mask[w] = 0u;
  __syncthreads();
  for (int64_t k = t; k < len; k += 256) {
    const int32_t row = members[beg + k];
    if (row < 0 || row >= G) { atomicOr(status, GV_ST_RANGE); continue; }
    const uint32_t bit = 1u << (row & 31);
    if (atomicOr(&s_mask[row >> 5], bit) & bit) atomicOr(status, GV_ST_DUP);
  }
  for (int c = 0; c < C; ++c) {
    const int32_t* col = kept + (int64_t)c * G;
    int32_t cnt = 0;
    for (int64_t k = t; k < len; k += 256) {
      const int32_t row = members[beg + k];
      if (row >= 0 && row < G) cnt += col[row] != 0 ? 1 : 0;
    }
    cnt = gficf_wave_sum(cnt);
    __syncthreads();
    if ((t & 63) == 0) s_c[t >> 6] = cnt;
    __syncthreads();
    if (t == 0) {
      const int64_t m = s_c[0] + s_c[1] + s_c[2] + s_c[3], top = hi < (int64_t)gc[c] - 1 ? hi : (int64_t)gc[c] - 1;
      msize[(int64_t)c * P + p] = (int32_t)m;
      tested[(int64_t)c * P + p] = (n_c[c] >= 2 && m >= 1 && m >= lo && m <= top) ? 1 : 0;
    }
  }
}

// One workgroup per cell j of cluster c.  LDS lists of the cell's n stored kept genes (dynamic, npad entries each):
//   A     their ranks in the cluster's d0 order, ascending
//   posA  the position of the gene of A[i] in this cell's order
//   Bk,Bg their real keys and rows, ascending by (key, row)
// then the mask of G_c bits.
__global__ __launch_bounds__(256) void k_gv_walk(int32_t G, int32_t C, int64_t P, int32_t npad, const int32_t* __restrict__ cluster,
                                                 const int64_t* __restrict__ colptr, const int32_t* __restrict__ row, const int64_t* __restrict__ src,
                                                 int64_t nnz, const double* __restrict__ dnz, const double* __restrict__ d0,
                                                 const int32_t* __restrict__ kept, const int32_t* __restrict__ gc, const int32_t* __restrict__ rank,
                                                 const u64* __restrict__ skey, const uint32_t* __restrict__ order, const int64_t* __restrict__ ptr,
                                                 const int32_t* __restrict__ members, const int32_t* __restrict__ msize,
                                                 const int32_t* __restrict__ tested, double* __restrict__ es, uint32_t* __restrict__ status) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char gv_lds[];
  u64* Bk = (u64*)gv_lds;
  uint32_t* A = (uint32_t*)(Bk + npad);
  int32_t* posA = (int32_t*)(A + npad);
  int32_t* Bg = posA + npad;
  uint32_t* s_mask = (uint32_t*)(Bg + npad);
  __shared__ int32_t s_n;
  __shared__ int32_t s_cnt[4];
  __shared__ double s_w[4], s_max[4], s_min[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t j = blockIdx.x;
  const int32_t c = cluster[j];
  if (c < 0 || c >= C) return;                             // flagged by k_gv_count
  const int32_t Gc = gc[c];
  if (Gc < 2) return;                                      // nothing is tested in this cluster
  const int64_t beg = colptr[j], end = colptr[j + 1];
  if (beg < 0 || end < beg || end > nnz || end - beg > (int64_t)npad) {
    if (t == 0) atomicOr(status, GV_ST_PTR);
    return;
  }
  const int64_t cg = (int64_t)c * G;
  if (t == 0) s_n = 0;
  __syncthreads();
  for (int64_t e = beg + t; e < end; e += 256) {
    const int32_t g = row[e];
    const int64_t si = src[e];
    if (g < 0 || g >= G || si < 0 || si >= nnz) { atomicOr(status, GV_ST_INDEX); continue; }
    if (e > beg && row[e - 1] >= g) atomicOr(status, GV_ST_INDEX);
    if (kept[cg + g] == 0) continue;
    const double v = dnz[si];
    if (!isfinite(v)) atomicOr(status, GV_ST_VALUE);
    const int i = atomicAdd(&s_n, 1);                      // any slot: the sorts below fix the order (no two entries compare equal)
    A[i] = (uint32_t)rank[cg + g];
    Bk[i] = ~gficf_f64_key(v);                             // descending, as the cluster's order of the d0
    Bg[i] = g;
  }
  __syncthreads();
  const int n = s_n;
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int i = n + t; i < np2; i += 256) { A[i] = 0xffffffffu; Bk[i] = ~0ull; Bg[i] = 0x7fffffff; }
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1) {
    for (int h = k >> 1; h > 0; h >>= 1) {
      for (int i = t; i < np2; i += 256) {
        const int l = i ^ h;
        if (l > i) {
          const bool up = (i & k) == 0;
          const uint32_t a0 = A[i], a1 = A[l];
          if ((a0 > a1) == up) { A[i] = a1; A[l] = a0; }
          const u64 k0 = Bk[i], k1 = Bk[l];
          const int32_t g0 = Bg[i], g1 = Bg[l];
          const bool gt = k0 > k1 || (k0 == k1 && g0 > g1);
          if (gt == up) { Bk[i] = k1; Bk[l] = k0; Bg[i] = g1; Bg[l] = g0; }
        }
      }
      __syncthreads();
    }
  }
  // the position of every stored kept gene: the kept genes whose d0 key precedes its real key (a search in the cluster's
  // order), less the stored ones among them, plus the stored ones whose real key precedes it (its place in B)
  for (int b = t; b < n; b += 256) {
    const u64 kq = Bk[b];
    const int32_t g = Bg[b];
    int lo = 0, hi = Gc;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const u64 km = skey[cg + mid];
      const int32_t gm = (int32_t)((int64_t)order[cg + mid] - cg);
      if (km < kq || (km == kq && gm < g)) lo = mid + 1; else hi = mid;
    }
    const int ia = gficf_lower_bound(A, n, (uint32_t)rank[cg + g]);
    if (ia < n) posA[ia] = lo - gficf_lower_bound(A, n, (uint32_t)lo) + b;
  }
  __syncthreads();
  const int W = (Gc + 31) >> 5;
  const int wpt = ((W + 255) >> 8) | 1;
  const int w0 = t * wpt < W ? t * wpt : W, w1 = w0 + wpt < W ? w0 + wpt : W;
  const double half_g = (double)Gc / 2.0;
  for (int64_t p = 0; p < P; ++p) {
    if (tested[(int64_t)c * P + p] == 0) continue;
    const int32_t m = msize[(int64_t)c * P + p];
    const int64_t pb = ptr[p], pl = ptr[p + 1] - pb;
    for (int w = t; w < W; w += 256) s_mask[w] = 0u;
    __syncthreads();
    for (int64_t k = t; k < pl; k += 256) {
      const int32_t g = members[pb + k];
      if (g < 0 || g >= G || kept[cg + g] == 0) continue;
      const uint32_t r0 = (uint32_t)rank[cg + g];
      const int ia = gficf_lower_bound(A, n, r0);
      int pos;
      if (ia < n && A[ia] == r0) {
        pos = posA[ia];
      } else {
        const u64 kq = ~gficf_f64_key(d0[cg + g]);
        int lo = 0, hi = n;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          const u64 km = Bk[mid];
          if (km < kq || (km == kq && Bg[mid] < g)) lo = mid + 1; else hi = mid;
        }
        pos = (int)r0 - ia + lo;
      }
      if (pos >= 0 && pos < Gc) atomicOr(&s_mask[pos >> 5], 1u << (pos & 31));
    }
    __syncthreads();
    int32_t cnt = 0;
    double wl = 0.0;
    for (int w = w0; w < w1; ++w) {
      uint32_t bits = s_mask[w];
      cnt += __popc(bits);
      while (bits) {
        const int32_t S = (w << 5) + __builtin_ctz(bits) + 1;
        bits &= bits - 1u;
        wl += fabs((double)(Gc - S + 1) - half_g);
      }
    }
    int32_t incl = cnt;                                    // inclusive scans over the wave, then the waves' totals through LDS
    double winc = wl;                                      // (multiples of 0.5: exact in any order)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t up = __shfl_up(incl, d);
      const double wu = __shfl_up(winc, d);
      if (lane >= d) { incl += up; winc += wu; }
    }
    if (lane == 63) { s_cnt[wave] = incl; s_w[wave] = winc; }
    __syncthreads();
    int32_t i = incl - cnt, total = 0;
    double cum = winc - wl, Wt = 0.0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (v < wave) { i += s_cnt[v]; cum += s_w[v]; }
      total += s_cnt[v];
      Wt += s_w[v];
    }
    if (t == 0 && total != m) atomicOr(status, GV_ST_DUP);
    const double dgm = (double)(Gc - m);
    double mx = -INFINITY, mn = INFINITY;
    for (int w = w0; w < w1; ++w) {
      uint32_t bits = s_mask[w];
      while (bits) {
        const int32_t S = (w << 5) + __builtin_ctz(bits) + 1;  // 1-based position
        bits &= bits - 1u;
        ++i;
        const double q = (double)(S - i) / dgm;
        const double bottom = cum / Wt - q;
        cum += fabs((double)(Gc - S + 1) - half_g);
        const double top = cum / Wt - q;
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
      es[j * P + p] = Wt == 0.0 ? (double)NAN : fmax(0.0, maxP) + fmin(0.0, minP);
    }
  }
}

// thread (p, c): block x covers 256 pathways, block y is the cluster
__global__ __launch_bounds__(256) void k_gv_sums(int64_t N, int64_t P, const int32_t* __restrict__ cluster, const double* __restrict__ es,
                                                 double* __restrict__ sum, double* __restrict__ sumsq) {
#pragma clang fp contract(off)
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int32_t c = (int32_t)blockIdx.y;
  if (p >= P) return;
  double s = 0.0, q = 0.0;
  for (int64_t j = 0; j < N; ++j) {
    if (cluster[j] != c) continue;
    const double y = es[j * P + p];
    s += y;
    q += y * y;
  }
  sum[(int64_t)c * P + p] = s;
  sumsq[(int64_t)c * P + p] = q;
}

// ------------------------------------------------------- workspace
struct GvWs {
  uint32_t* status;
  int32_t *n_c, *gc;
  gficf_sort_bufs sort;
  u64* skey;
  int32_t *rank, *msize;
};

static size_t gv_carve(char* base, int64_t G, int64_t C, int64_t P, GvWs& w) {
  gficf_carver cv;
  cv.base = base;
  const size_t gc = (size_t)std::max<int64_t>(G * C, 1);
  w.status = cv.take<uint32_t>(1);
  w.n_c = cv.take<int32_t>((size_t)C);
  w.gc = cv.take<int32_t>((size_t)C);
  w.sort.take(cv, gc, gc, {gficf_bit_width(C - 1)});
  w.skey = cv.take<u64>(gc);
  w.rank = cv.take<int32_t>(gc);
  w.msize = cv.take<int32_t>((size_t)std::max<int64_t>(P * C, 1));
  return cv.total();
}

static int gv_check_sizes(int64_t G, int64_t N, int64_t C, int64_t P) {
  if (G < 1 || N < 1 || C < 1 || P < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld, C = %lld, P = %lld: a size is out of range", (long long)G, (long long)N, (long long)C, (long long)P);
  if (G > GFICF_GSVA_MAX_G) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "G = %lld genes: the LDS position mask holds %d", (long long)G, GFICF_GSVA_MAX_G);
  if (N > INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^31 - 1 cells");
  if (C > 65535) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 65 535 clusters");
  if (G * C > INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^31 - 1 (gene, cluster) pairs");
  if ((double)P * (double)C > (double)INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^31 - 1 (pathway, cluster) pairs");
  return GFICF_OK;
}

static int gv_workspace(void* ws, size_t ws_bytes, int64_t G, int64_t C, int64_t P, GvWs& w) {
  if (!ws) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL workspace");
  return gficf_addon_carve(ws, ws_bytes, [&](char* base) { return gv_carve(base, G, C, P, w); });
}

// n_c of every cluster into w.n_c
static int gv_count(gficf_ctx* ctx, const GvWs& w, int64_t N, int32_t C, const int32_t* d_cluster) {
  GFICF_HIP_CHECK(hipMemsetAsync(w.n_c, 0, sizeof(int32_t) * (size_t)C, ctx->stream));
  hipLaunchKernelGGL(k_gv_count, dim3(gficf_grid_1d(N)), dim3(256), 0, ctx->stream, N, C, d_cluster, w.n_c, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

static int npad_of(int64_t max_cell_nz) {
  int np = 64;
  while (np < max_cell_nz) np <<= 1;
  return np;
}

}  // namespace

extern "C" {

int gficf_gsva_abi_version(void) { return GFICF_GSVA_ABI_VERSION; }

size_t gficf_gsva_workspace_bytes(int64_t G, int64_t N, int32_t C, int64_t P) {
  if (G < 1 || N < 1 || C < 1 || P < 0 || G > GFICF_GSVA_MAX_G || G * (int64_t)C > INT32_MAX || (double)P * (double)C > (double)INT32_MAX) return 0;
  GvWs w;
  return gv_carve(nullptr, G, C, P, w);
}

int gficf_gsva_density_device(gficf_ctx* ctx, int64_t G, int64_t N, int32_t C, const int32_t* d_cluster, const int64_t* d_seg_ptr,
                              const int32_t* d_cell, const double* d_x, int64_t nnz, int64_t max_seg, void* ws, size_t ws_bytes, double* d_sd,
                              double* d_d0, int32_t* d_kept, double* d_dnz) {
  GFICF_CTX_ENTER(ctx);
  int rc = gv_check_sizes(G, N, C, 0);
  if (rc) return rc;
  if (nnz < 0 || max_seg < 0 || max_seg > N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "nnz = %lld, max_seg = %lld", (long long)nnz, (long long)max_seg);
  if (!d_cluster || !d_seg_ptr || !d_sd || !d_d0 || !d_kept || (nnz > 0 && (!d_cell || !d_x || !d_dnz))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  GvWs w;
  rc = gv_workspace(ws, ws_bytes, G, C, 0, w);
  if (rc) return rc;
  const int64_t splits = std::max<int64_t>(gficf_ceil_div(max_seg, GFICF_GSVA_JSPLIT), 1);
  if (splits > 65535) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "a segment of %lld entries", (long long)max_seg);
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), ctx->stream));
  rc = gv_count(ctx, w, N, C, d_cluster);
  if (rc) return rc;
  hipLaunchKernelGGL(k_gv_density, dim3((unsigned)(G * C), (unsigned)splits), dim3(256), 0, ctx->stream, N, C, d_cluster, (const int32_t*)w.n_c, d_seg_ptr,
                     d_cell, d_x, nnz, d_sd, d_d0, d_kept, d_dnz, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_gsva_scores_device(gficf_ctx* ctx, int64_t G, int64_t N, int32_t C, const int32_t* d_cluster, const int64_t* d_colptr, const int32_t* d_row,
                             const int64_t* d_src, int64_t nnz, int64_t max_cell_nz, const double* d_dnz, const double* d_d0, const int32_t* d_kept,
                             int64_t P, const int64_t* d_ptr, const int32_t* d_members, int64_t n_members, int64_t min_size, int64_t max_size,
                             int32_t fresh, void* ws, size_t ws_bytes, double* d_es, int32_t* d_tested, double* d_sum, double* d_sumsq) {
  GFICF_CTX_ENTER(ctx);
  int rc = gv_check_sizes(G, N, C, P);
  if (rc) return rc;
  if (nnz < 0 || n_members < 0 || max_cell_nz < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "nnz = %lld, n_members = %lld, max_cell_nz = %lld", (long long)nnz, (long long)n_members, (long long)max_cell_nz);
  if (max_cell_nz > GFICF_GSVA_MAX_CELL_NZ)
    GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "a cell with %lld stored entries: the LDS lists hold %d", (long long)max_cell_nz, GFICF_GSVA_MAX_CELL_NZ);
  if (!d_cluster || !d_colptr || !d_d0 || !d_kept || !d_ptr || (nnz > 0 && (!d_row || !d_src || !d_dnz)) || (n_members > 0 && !d_members) ||
      (P > 0 && (!d_es || !d_tested || !d_sum || !d_sumsq)))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  GvWs w;
  rc = gv_workspace(ws, ws_bytes, G, C, P, w);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  if (fresh) GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), st));
  if (P == 0) return GFICF_OK;
  rc = gv_count(ctx, w, N, C, d_cluster);
  if (rc) return rc;
  const int64_t gc = G * C;
  hipLaunchKernelGGL(k_gv_gc, dim3((unsigned)C), dim3(256), 0, st, G, d_kept, w.gc);
  GFICF_HIP_CHECK(hipGetLastError());
  rc = gficf_sort_f64(ctx, w.sort, gc, {d_d0, 1, d_kept, w.status, GV_ST_VALUE, nullptr, nullptr, (uint32_t)G, gficf_bit_width(C - 1)});   // (cluster, d0 desc, row) order
  if (rc) return rc;
  hipLaunchKernelGGL(k_gv_rank, dim3(gficf_grid_1d(gc)), dim3(256), 0, st, gc, (uint32_t)G, (const uint32_t*)w.sort.oval, (const u64*)w.sort.key, w.rank, w.skey);
  const int64_t lo = min_size > 1 ? min_size : 1, hi = max_size < G ? max_size : G;
  hipLaunchKernelGGL(k_gv_sizes, dim3((unsigned)P), dim3(256), 0, st, (int32_t)G, C, P, d_ptr, n_members, d_members, d_kept, (const int32_t*)w.n_c,
                     (const int32_t*)w.gc, lo, hi, w.msize, d_tested, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  GFICF_HIP_CHECK(hipMemsetAsync(d_es, 0, sizeof(double) * (size_t)P * (size_t)N, st));
  const int npad = npad_of(max_cell_nz);
  const size_t lds = (size_t)npad * 20 + (size_t)((G + 31) / 32) * sizeof(uint32_t);
  GFICF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_gv_walk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_gv_walk, dim3((unsigned)N), dim3(256), lds, st, (int32_t)G, C, P, (int32_t)npad, d_cluster, d_colptr, d_row, d_src, nnz, d_dnz, d_d0,
                     d_kept, (const int32_t*)w.gc, (const int32_t*)w.rank, (const u64*)w.skey, (const uint32_t*)w.sort.oval, d_ptr, d_members,
                     (const int32_t*)w.msize, (const int32_t*)d_tested, d_es, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_gv_sums, dim3((unsigned)gficf_ceil_div(P, 256), (unsigned)C), dim3(256), 0, st, N, P, d_cluster, (const double*)d_es, d_sum, d_sumsq);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_gsva_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  const int rc = gficf_addon_read_status(ctx, ws, &st);
  if (rc) return rc;
  if (st & GV_ST_CLUSTER) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a cluster id outside [0, C)");
  if (st & GV_ST_PTR) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "offsets that decrease or leave their array, or a cell longer than announced");
  if (st & GV_ST_INDEX) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a cell, row or src index out of range, or rows of a cell that do not ascend");
  if (st & GV_ST_GROUP) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a segment holds an entry of another cluster's cell, or more entries than its cluster has cells");
  if (st & GV_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "the matrix or the densities hold a NaN or an infinite value");
  if (st & GV_ST_RANGE) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a pathway member outside [0, G)");
  if (st & GV_ST_DUP) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a member repeated within a pathway");
  return GFICF_OK;
}

}  // extern "C"

namespace {

// what the two host entries share: the pathway offsets and the cell-major offsets checked on the host (they size copies and launches)
static int gv_host_offsets(const int64_t* p, int64_t n, const char* what, int64_t* last, int64_t* longest) {
  if (!p) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "%s is NULL", what);
  if (p[0] != 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "%s[0] = %lld, expected 0", what, (long long)p[0]);
  int64_t mx = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (p[i + 1] < p[i]) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "%s decreases at position %lld", what, (long long)(i + 1));
    mx = std::max(mx, p[i + 1] - p[i]);
  }
  *last = p[n];
  if (longest) *longest = mx;
  return GFICF_OK;
}

// both host entries: dens == true runs stages 1-2 first (seg_ptr, cell, x given), else dnz, d0 and kept are inputs
static int gv_host(gficf_ctx* ctx, bool dens, int64_t G, int64_t N, int32_t C, const int32_t* cluster, const int64_t* seg_ptr, const int32_t* cell,
                   const double* x, const int64_t* colptr, const int32_t* row, const int64_t* src, int64_t nnz_in, double* dnz, double* d0, int32_t* kept,
                   double* sd, int64_t P, const int64_t* ptr, const int32_t* members, int64_t min_size, int64_t max_size, double* es, int32_t* tested,
                   double* sum, double* sumsq) {
  GFICF_CTX_ENTER(ctx);
  int rc = gv_check_sizes(G, N, C, P);
  if (rc) return rc;
  int64_t nm = 0, nnz = 0, max_cell = 0, max_seg = 0, nnz_seg = 0;
  rc = gv_host_offsets(ptr, P, "ptr", &nm, nullptr);
  if (rc) return rc;
  rc = gv_host_offsets(colptr, N, "colptr", &nnz, &max_cell);
  if (rc) return rc;
  if (dens) {
    rc = gv_host_offsets(seg_ptr, G * C, "seg_ptr", &nnz_seg, &max_seg);
    if (rc) return rc;
    if (nnz_seg != nnz) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "seg_ptr ends at %lld entries, colptr at %lld", (long long)nnz_seg, (long long)nnz);
    if (max_seg > N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a segment of %lld entries, but %lld cells", (long long)max_seg, (long long)N);
  } else if (nnz != nnz_in) {
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "colptr ends at %lld entries, nnz = %lld", (long long)nnz, (long long)nnz_in);
  }
  if (max_cell > GFICF_GSVA_MAX_CELL_NZ)
    GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "a cell with %lld stored entries: the LDS lists hold %d", (long long)max_cell, GFICF_GSVA_MAX_CELL_NZ);
  if (!cluster || !kept || (P > 0 && (!es || !tested || !sum || !sumsq)) || (nm > 0 && !members) || (nnz > 0 && (!row || !src)) ||
      (dens ? (nnz > 0 && (!cell || !x)) : (!d0 || (nnz > 0 && !dnz))))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t gc = (size_t)(G * C), pc = (size_t)(P * C), pn = (size_t)P * (size_t)N, ne = (size_t)(nnz > 0 ? nnz : 1);
  const size_t wsb = gficf_gsva_workspace_bytes(G, N, C, P);
  gficf_host_io io{ctx, dens ? "gficf_gsva_host" : "gficf_gsva_scores_host"};
  gficf_carver cv;
  int32_t *d_cl, *d_cell, *d_row, *d_mem, *d_kept, *d_tst; int64_t *d_seg, *d_col, *d_src, *d_ptr; double *d_x, *d_dnz, *d_d0, *d_sd, *d_es, *d_sum, *d_sq; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_cl = cv.take<int32_t>((size_t)N); d_seg = cv.take<int64_t>(dens ? gc + 1 : 1); d_cell = cv.take<int32_t>(dens ? ne : 1); d_x = cv.take<double>(dens ? ne : 1);
    d_col = cv.take<int64_t>((size_t)N + 1); d_row = cv.take<int32_t>(ne); d_src = cv.take<int64_t>(ne);
    d_ptr = cv.take<int64_t>((size_t)P + 1); d_mem = cv.take<int32_t>((size_t)(nm > 0 ? nm : 1));
    d_dnz = cv.take<double>(ne); d_d0 = cv.take<double>(gc); d_sd = cv.take<double>(gc); d_kept = cv.take<int32_t>(gc);
    d_es = cv.take<double>(pn ? pn : 1); d_tst = cv.take<int32_t>(pc ? pc : 1); d_sum = cv.take<double>(pc ? pc : 1); d_sq = cv.take<double>(pc ? pc : 1);
    d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_cl, cluster, sizeof(int32_t) * (size_t)N);
  io.up(d_col, colptr, sizeof(int64_t) * ((size_t)N + 1));
  io.up(d_row, row, sizeof(int32_t) * (size_t)nnz);
  io.up(d_src, src, sizeof(int64_t) * (size_t)nnz);
  io.up(d_ptr, ptr, sizeof(int64_t) * ((size_t)P + 1));
  io.up(d_mem, members, sizeof(int32_t) * (size_t)nm);
  if (dens) {
    io.up(d_seg, seg_ptr, sizeof(int64_t) * (gc + 1));
    io.up(d_cell, cell, sizeof(int32_t) * (size_t)nnz);
    io.up(d_x, x, sizeof(double) * (size_t)nnz);
  } else {
    io.up(d_dnz, dnz, sizeof(double) * (size_t)nnz);
    io.up(d_d0, d0, sizeof(double) * gc);
    io.up(d_kept, kept, sizeof(int32_t) * gc);
  }
  if (io.ok()) {
    if (dens) rc = gficf_gsva_density_device(ctx, G, N, C, d_cl, d_seg, d_cell, d_x, nnz, max_seg, d_ws, wsb, d_sd, d_d0, d_kept, d_dnz);
    if (!rc)
      rc = gficf_gsva_scores_device(ctx, G, N, C, d_cl, d_col, d_row, d_src, nnz, max_cell, d_dnz, d_d0, d_kept, P, d_ptr, d_mem, nm, min_size, max_size,
                                    dens ? 0 : 1, d_ws, wsb, d_es, d_tst, d_sum, d_sq);
    if (!rc) {
      io.down(es, d_es, sizeof(double) * pn);
      io.down(tested, d_tst, sizeof(int32_t) * pc);
      io.down(sum, d_sum, sizeof(double) * pc);
      io.down(sumsq, d_sq, sizeof(double) * pc);
      if (dens) {
        io.down(kept, d_kept, sizeof(int32_t) * gc);
        if (sd) io.down(sd, d_sd, sizeof(double) * gc);
        if (d0) io.down(d0, d_d0, sizeof(double) * gc);
        if (dnz) io.down(dnz, d_dnz, sizeof(double) * (size_t)nnz);
      }
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_gsva_sync(ctx, d_ws);
}

}  // namespace

extern "C" {

int gficf_gsva_host(gficf_ctx* ctx, int64_t G, int64_t N, int32_t C, const int32_t* cluster, const int64_t* seg_ptr, const int32_t* cell,
                    const double* x, const int64_t* colptr, const int32_t* row, const int64_t* src, int64_t P, const int64_t* ptr,
                    const int32_t* members, int64_t min_size, int64_t max_size, double* es, int32_t* tested, int32_t* kept, double* sd, double* d0,
                    double* dnz, double* sum, double* sumsq) {
  return gv_host(ctx, true, G, N, C, cluster, seg_ptr, cell, x, colptr, row, src, 0, dnz, d0, kept, sd, P, ptr, members, min_size, max_size, es, tested, sum,
                 sumsq);
}

int gficf_gsva_scores_host(gficf_ctx* ctx, int64_t G, int64_t N, int32_t C, const int32_t* cluster, const int64_t* colptr, const int32_t* row,
                           const int64_t* src, int64_t nnz, const double* dnz, const double* d0, const int32_t* kept, int64_t P, const int64_t* ptr,
                           const int32_t* members, int64_t min_size, int64_t max_size, double* es, int32_t* tested, double* sum, double* sumsq) {
  return gv_host(ctx, false, G, N, C, cluster, nullptr, nullptr, nullptr, colptr, row, src, nnz, const_cast<double*>(dnz), const_cast<double*>(d0),
                 const_cast<int32_t*>(kept), nullptr, P, ptr, members, min_size, max_size, es, tested, sum, sumsq);
}

}  // extern "C"
